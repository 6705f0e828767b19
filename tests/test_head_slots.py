"""mgx_spmm_copy_u_slots_init: mgx_spmm_copy_u_strided_init with the gathered matrix's 128-byte slots beside it -- compared on bit
patterns (int32 views) with that call on the same graph and plan, over a hand-made graph whose in-degrees sit on every boundary of the
kernel (the four accumulators, eight slots per instruction, a step of 16, the chunk of 64, the 256-edge partials of split rows and their
fix-up), three plan forms, source matrices from all-zero to all-dense and three initial-value lists; the documented exception (-0.0f
operands: equal as numbers); what the entry point refuses; mgx_rows_slots_pack_rows against the whole-matrix pack; and the layer that
uses both (ops.SageMeanCatHeadFn, config.SAGE_HEAD_SLOTS) against itself with the switch off over three steps whose row list changes,
and inside a captured step."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dgl-0.5-benchmark_amd")
sys.path.insert(0, PKG)
import mi355x_graph as mg  # noqa: E402
from mi355x_graph import _lib, config, ops, schedule, sparse  # noqa: E402
from conftest import random_graph  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, D = 4096, 64
DEGREES = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257]
HUB = 1003
LONELY = 77   # the node with no out-edges


def _be():
    return sparse.backend_for(torch.zeros(1, device=DEV))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _edges():
    """In-degrees cycling through DEGREES in a shuffled order, the hub of HUB edges as the last row; sources anywhere but LONELY."""
    rng = np.random.default_rng(11)
    deg = np.array([DEGREES[i % len(DEGREES)] for i in range(N)], dtype=np.int64)
    rng.shuffle(deg)
    deg[N - 1] = HUB
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, N - 1, int(indptr[-1]))
    indices[indices >= LONELY] += 1
    assert set(DEGREES) <= set(deg.tolist()) and not (indices == LONELY).any() and indices.max() == N - 1
    return indptr, indices


def _csr(form, monkeypatch):
    indptr, indices = _edges()
    if form == "cluster":
        monkeypatch.setenv("MGX_SCHEDULE", "cluster")
    csr = sparse.CsrView(N, N, torch.from_numpy(indptr).to(torch.int32).to(DEV), torch.from_numpy(indices).to(torch.int32).to(DEV), None)
    plan = csr.plan()
    assert plan is not None and plan.num_hubs >= 3 and plan.order_kind == ("cluster" if form == "cluster" else "natural")
    if form == "two-part":   # forced the way tests/test_rowgroup_spmm.py forces one
        split = schedule.split_short_items(csr, plan, any_share=True, limit=16)
        assert split is not None and split[0].rest is not None and split[0].rest.num_hubs >= 3
        csr._short = {nb: split[0] for nb in (2, 4, 8, 16, 32, 64)}
        assert csr.spmm_plan_for(D) == (split[0], True)
    else:
        csr._short = {nb: None for nb in (2, 4, 8, 16, 32, 64)}
        assert csr.spmm_plan_for(D) == (plan, False)
    assert csr.tile_plan(D) is None
    return csr


def _sources():
    gen = torch.Generator(device=DEV).manual_seed(5)
    dense = torch.randn(N, D, device=DEV, generator=gen)
    dense[dense == 0] = 1.0
    pick = torch.rand(N, device=DEV, generator=gen) < 0.08
    rows8 = dense * pick.view(-1, 1)
    rows8[~pick] = 0.0
    sparse20 = dense * (torch.rand(N, D, device=DEV, generator=gen) < 0.2)
    sparse20[sparse20 == 0] = 0.0   # (no -0.0f from the product with a zero mask)
    counted = torch.zeros(N, D, device=DEV)
    for i, k in enumerate((1, 24, 25)):   # rows of exactly 1, 24 and 25 non-zeros, at random columns: the slot's capacity from both sides
        r = torch.arange(i, N, 3, device=DEV)
        cols = torch.rand(r.shape[0], D, device=DEV, generator=gen).argsort(dim=1)[:, :k]
        counted[r.view(-1, 1), cols] = dense[r.view(-1, 1), cols]
    special = rows8.clone()
    live = torch.nonzero(pick).flatten()
    special[live[0::5], 3] = float("inf")
    special[live[1::5], 40] = float("-inf")
    special[live[2::5], 63] = float("nan")
    return {"zero": torch.zeros(N, D, device=DEV), "dense": dense, "8 percent rows": rows8, "20 percent": sparse20,
            "1 / 24 / 25 non-zeros": counted, "inf and nan": special}


def _lists():
    gen = torch.Generator(device=DEV).manual_seed(6)
    perm = torch.randperm(N, device=DEV, generator=gen)
    some = perm[:N * 8 // 100]
    some = torch.cat([some[some != N - 1], torch.tensor([N - 1], device=DEV)]).contiguous()   # unsorted, distinct, the hub row among them
    return {"empty": torch.zeros(0, dtype=torch.int64, device=DEV), "all": torch.arange(N, device=DEV), "8 percent": some}


def _pos(rows, n=N):
    pos = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    pos[rows] = torch.arange(rows.shape[0], dtype=torch.int64, device=DEV)
    return pos


def _last_kernel():
    return _lib.lib().mgx_last_spmm_kernel()


@pytest.mark.parametrize("form", ["natural", "cluster", "two-part"])
def test_bits_of_the_dense_call(form, monkeypatch):
    be, csr = _be(), _csr(form, monkeypatch)
    lists = _lists()
    assert int((_pos(lists["8 percent"]) >= 0).sum()) == lists["8 percent"].shape[0] and bool((lists["8 percent"] == N - 1).any())
    gen = torch.Generator(device=DEV).manual_seed(7)
    for sname, u in _sources().items():
        slots, overflow = be.rows_slots_pack(u)
        if sname == "dense":
            assert int(overflow) == N
        for lname, rows in lists.items():
            init = torch.randn(rows.shape[0], D, device=DEV, generator=gen)
            pos = _pos(rows)
            want = be.spmm_copy_u_strided_init(csr, "sum", u, init, pos, torch.full((N, D), float("nan"), device=DEV))
            assert want is not None and _last_kernel() == (b"rowgroup32" if form == "two-part" else b"rowwave32")
            out = torch.full((N, D), float("nan"), device=DEV)
            sparse.PROFILE = []
            try:
                got = be.spmm_copy_u_slots_init(csr, "sum", u, slots, init, pos, out)
            finally:
                recs, sparse.PROFILE = sparse.PROFILE, None
            assert got is out and _last_kernel() == b"slots"
            assert len(recs) == 1 and "slots" in recs[0]["variant"].split("+") and recs[0]["accumulate"] is True
            diff = torch.nonzero((_bits(got) != _bits(want)).any(dim=1)).flatten()
            print("%s / %s / %s: %d rows differ" % (form, sname, lname, diff.numel()))
            assert diff.numel() == 0, (form, sname, lname, diff[:10].tolist())
            if sname == "zero" and lname == "empty":
                assert bool((_bits(got) == 0).all())


def test_row_strides_of_all_three_matrices(monkeypatch):
    be, csr = _be(), _csr("two-part", monkeypatch)
    u = _sources()["8 percent rows"]
    rows = _lists()["8 percent"]
    gen = torch.Generator(device=DEV).manual_seed(8)
    wide_init = torch.randn(rows.shape[0], 128, device=DEV, generator=gen)
    init = wide_init[:, 64:]                                   # row stride 128 floats
    wide_u = torch.full((N, 128), float("nan"), device=DEV)
    wide_u[:, 32:96] = u
    wide_out = torch.full((N, 192), float("nan"), device=DEV)
    out = wide_out[:, 64:128]
    pos = _pos(rows)
    want = be.spmm_copy_u_strided_init(csr, "sum", u, init.contiguous(), pos, torch.empty(N, D, device=DEV))
    for src in (u, wide_u[:, 32:96]):                          # row strides 64 and 128
        wide_out.fill_(float("nan"))
        slots = be.rows_slots_pack(src)[0]
        got = be.spmm_copy_u_slots_init(csr, "sum", src, slots, init, pos, out)
        assert got is out and _last_kernel() == b"slots" and torch.equal(_bits(got), _bits(want))
        assert bool(torch.isnan(wide_out[:, :64]).all()) and bool(torch.isnan(wide_out[:, 128:]).all())   # nothing written beside it


@pytest.mark.parametrize("form", ["natural", "two-part"])
def test_negative_zeros_are_equal_as_numbers(form, monkeypatch):
    """The documented exception: the pack drops a -0.0f and a skipped +0.0f addend would have cleared the sign of a -0.0f sum, so with
    -0.0f in the operands only the sign of an exactly-zero result may differ."""
    be, csr = _be(), _csr(form, monkeypatch)
    gen = torch.Generator(device=DEV).manual_seed(9)
    u = _sources()["20 percent"].clone()
    u[torch.rand(N, D, device=DEV, generator=gen) < 0.1] = -0.0
    u[::7] = -0.0
    rows = _lists()["8 percent"]
    init = torch.randn(rows.shape[0], D, device=DEV, generator=gen)
    init[torch.rand(init.shape, device=DEV, generator=gen) < 0.2] = -0.0
    init[0] = -0.0
    pos = _pos(rows)
    want = be.spmm_copy_u_strided_init(csr, "sum", u, init, pos, torch.empty(N, D, device=DEV))
    got = be.spmm_copy_u_slots_init(csr, "sum", u, be.rows_slots_pack(u)[0], init, pos, torch.empty(N, D, device=DEV))
    assert _last_kernel() == b"slots"
    assert torch.equal(got, want)
    differ = _bits(got) != _bits(want)
    assert bool((want[differ] == 0).all())


def test_refusals_leave_the_output_alone(monkeypatch):
    be, csr = _be(), _csr("natural", monkeypatch)
    u = _sources()["8 percent rows"]
    slots = be.rows_slots_pack(u)[0]
    rows = _lists()["8 percent"]
    init = torch.randn(rows.shape[0], D, device=DEV)
    pos = _pos(rows)
    out = torch.full((N, D), 7.0, device=DEV)
    assert be.spmm_copy_u_slots_init(csr, "mean", u, slots, init, pos, out) is None
    assert be.spmm_copy_u_slots_init(csr, "sum", u, slots, init, pos, out, dst_scale=torch.ones(N, device=DEV)) is None
    out60 = torch.full((N, 60), 7.0, device=DEV)
    assert be.spmm_copy_u_slots_init(csr, "sum", u[:, :60].contiguous(), slots, init[:, :60].contiguous(), pos, out60) is None
    u128, out128 = torch.randn(N, 128, device=DEV), torch.full((N, 128), 7.0, device=DEV)
    assert be.spmm_copy_u_slots_init(csr, "sum", u128, slots, torch.randn(rows.shape[0], 128, device=DEV), pos, out128) is None
    assert be.spmm_copy_u_slots_init(csr.astype(torch.int64), "sum", u, slots, init, pos, out) is None
    for bad in (slots[:-1], slots[:, :16].contiguous(), slots.to(torch.int64), torch.zeros(N, 64, dtype=torch.int32, device=DEV)[:, ::2]):
        with pytest.raises(mg.DGLError):
            be.spmm_copy_u_slots_init(csr, "sum", u, bad, init, pos, out)
    # the entry point itself, not the wrapper
    import ctypes
    st = _lib.lib().mgx_spmm_copy_u_slots_init(ctypes.byref(csr.c_struct()), None, _lib.REDUCE["mean"], u.data_ptr(), D, D, slots.data_ptr(), None,
                                               init.data_ptr(), rows.shape[0], D, pos.data_ptr(), out.data_ptr(), D, None, 0, None)
    assert st == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((out60 == 7.0).all()) and bool((out128 == 7.0).all())


@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, N])
def test_pack_rows_writes_the_listed_slots_and_no_other(count):
    be = _be()
    gen = torch.Generator(device=DEV).manual_seed(10 + count)
    wide = torch.full((N, 96), float("nan"), device=DEV)
    x = wide[:, 16:80]                                          # a row-strided view
    x.copy_(_sources()["1 / 24 / 25 non-zeros"])
    x[5::11] = torch.randn(x[5::11].shape, device=DEV, generator=gen)   # dense rows among them: flagged slots
    whole = be.rows_slots_pack(x)[0]
    rows = torch.randperm(N, device=DEV, generator=gen)[:count].contiguous()
    slots = torch.full((N, 32), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    assert be.rows_slots_pack_rows(x, rows, slots) is slots
    listed = torch.zeros(N, dtype=torch.bool, device=DEV)
    listed[rows] = True
    assert torch.equal(slots[listed], whole[listed])
    assert bool((slots[~listed] == 0x5a5a5a5a).all())


# ---- the layer
NL, RL = 65536, 5000   # the layer's gate (ops._ROWS_GEMM_MIN rows)


@pytest.fixture(scope="module")
def layer_world():
    src, dst = random_graph(NL, NL, 10 * NL, seed=31, skew=True)
    graphs = [mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=NL).int().formats(["csr", "csc"]).to(DEV) for _ in range(3)]
    gen = torch.Generator(device=DEV).manual_seed(8)
    perm = torch.randperm(NL, device=DEV, generator=gen)
    return {"g_on": graphs[0], "g_off": graphs[1], "g_cap": graphs[2], "h": torch.randn(NL, 64, device=DEV, generator=gen),
            "params": [torch.randn(47, 64, device=DEV, generator=gen) * 0.1, torch.randn(47, 64, device=DEV, generator=gen) * 0.1,
                       torch.randn(47, device=DEV, generator=gen)],
            "rows": [perm[:RL].contiguous(), perm[RL - 100:2 * RL - 100].contiguous()],   # two lists that share 100 rows
            "dyr": torch.randn(RL, 47, device=DEV, generator=gen)}


def _layer_grads(w, g, cat, rows, monkeypatch, on):
    monkeypatch.setattr(config, "SAGE_HEAD_SLOTS", on)
    h = w["h"].clone().requires_grad_(True)
    ws, wn, b = [p.clone().requires_grad_(True) for p in w["params"]]
    y = ops.SageMeanCatHeadFn.apply(g._index, cat, h, ws, wn, b, rows)
    y.backward(w["dyr"])
    return [h.grad, ws.grad, wn.grad, b.grad]


def _spy(monkeypatch, name):
    calls = []
    real = getattr(sparse.HipBackend, name)

    def spy(self, *a, **k):
        r = real(self, *a, **k)
        calls.append(r is not None)
        return r

    monkeypatch.setattr(sparse.HipBackend, name, spy)
    return calls


def test_layer_gives_the_same_four_gradients_with_the_switch_on_and_off(layer_world, monkeypatch):
    w = layer_world
    monkeypatch.setattr(config, "PACKED_GATHER_MIN_NNZ", 0)
    monkeypatch.delenv("MGX_SAGE_HEAD_SLOTS", raising=False)
    slot_calls, dense_calls = _spy(monkeypatch, "spmm_copy_u_slots_init"), _spy(monkeypatch, "spmm_copy_u_strided_init")
    cat_on, cat_off = ops.CatBuffer(NL, 64, DEV), ops.CatBuffer(NL, 64, DEV)
    second = w["rows"][1].clone()
    # step 1: a list; step 2: another tensor (the first list's rows are cleared, their slots must be empty again); step 3: that tensor
    # written in place (the whole matrix is cleared and packed again)
    for step, rows in enumerate((w["rows"][0], second, second)):
        if step == 2:
            second.copy_(torch.cat([w["rows"][0][:RL // 2], w["rows"][1][RL // 2:]]))
            assert second.unique().shape[0] == RL
        off = _layer_grads(w, w["g_off"], cat_off, rows, monkeypatch, False)
        assert slot_calls == [] and dense_calls == [True]
        dense_calls.clear()
        on = _layer_grads(w, w["g_on"], cat_on, rows, monkeypatch, True)
        assert slot_calls == [True] and dense_calls == []
        slot_calls.clear()
        for name, a_, b_ in zip(("d h", "d W_self", "d W_neigh", "d bias"), on, off):
            assert torch.equal(_bits(a_), _bits(b_)), (step, name, float((a_ - b_).abs().max()))
        # the slots kept beside the matrix are the matrix's, row for row
        buf, held_rows, _, slots = w["g_on"]._index.csr()._head_dn
        assert held_rows is rows and slots is not None and torch.equal(slots, _be().rows_slots_pack(buf)[0])
        assert int((buf != 0).any(dim=1).sum()) <= RL
    assert w["g_off"]._index.csr()._head_dn[3] is None
    # MGX_SAGE_HEAD_SLOTS=0, and a wrapper that declines: the dense call, the same gradients
    monkeypatch.setenv("MGX_SAGE_HEAD_SLOTS", "0")
    env_off = _layer_grads(w, w["g_on"], cat_on, second, monkeypatch, True)
    assert slot_calls == [] and dense_calls == [True]
    monkeypatch.delenv("MGX_SAGE_HEAD_SLOTS")
    monkeypatch.setattr(sparse.HipBackend, "spmm_copy_u_slots_init", lambda self, *a, **k: None)
    declined = _layer_grads(w, w["g_on"], cat_on, second, monkeypatch, True)
    assert dense_calls == [True, True]
    for grads in (env_off, declined):
        assert all(torch.equal(_bits(a_), _bits(b_)) for a_, b_ in zip(grads, off))


def test_layer_in_a_captured_step_takes_the_dense_call(layer_world, monkeypatch):
    from mi355x_graph.utils import GraphedStep
    w = layer_world
    monkeypatch.setattr(config, "PACKED_GATHER_MIN_NNZ", 0)
    rows = w["rows"][0]
    want = _layer_grads(w, w["g_off"], ops.CatBuffer(NL, 64, DEV), rows, monkeypatch, False)
    monkeypatch.setattr(config, "SAGE_HEAD_SLOTS", True)
    slot_calls, dense_calls = _spy(monkeypatch, "spmm_copy_u_slots_init"), _spy(monkeypatch, "spmm_copy_u_strided_init")
    leaves = [torch.nn.Parameter(t.clone()) for t in [w["h"]] + w["params"]]
    cat = ops.CatBuffer(NL, 64, DEV)

    def loss_fn():
        y = ops.SageMeanCatHeadFn.apply(w["g_cap"]._index, cat, leaves[0], leaves[1], leaves[2], leaves[3], rows)
        return (y * w["dyr"]).sum()

    step = GraphedStep(loss_fn, torch.optim.Adam(leaves, lr=0.0, capturable=True), warmup=2)
    n_eager = len(slot_calls)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    assert len(slot_calls) == n_eager and len(dense_calls) >= 1   # the capture itself took the dense call
    for name, p, b_ in zip(("d h", "d W_self", "d W_neigh", "d bias"), leaves, want):
        assert torch.equal(_bits(p.grad), _bits(b_)), (name, float((p.grad - b_).abs().max()))
