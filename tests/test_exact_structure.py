"""Exact-arithmetic structure tests: a lost, doubled or misattributed edge in ANY row is a mismatch.

Inputs are signed small integers stored as fp32 (zeros included), so every partial sum in any association is an integer below 2^24 and
the fp32 result does not depend on the summation order; the reference is numpy int64 arithmetic over the COO list.  Each case asserts
the precondition (sum of |terms| per output element < 2^24) from the reference alone, then compares `sum` bit for bit, `mean` within
4 ulp of float32(sum) / float32(deg), `max` / `min` and their arg indices exactly.  The graph is the degree ladder of exact_ladder.py:
row lengths on every chunk, tile, lane-group and 64-edge boundary the kernels have, hub rows first, last and adjacent, a hub source,
sources nobody gathers, duplicates, both id widths, square and bipartite.

CPU (no marker): the same cases on the OpenMP variants, the ladder through the three plan builders and tileplan.emulate, and the
comparator self-test that pins down why the 1e-4 relative bound cannot see a one-edge error on a long row.
GPU (-m gpu): every g-SpMM family forced and named through mgx_last_spmm_kernel(), edge softmax / GAT attention in their two exact
forms, the backward kernels against fp64 with the row-scaled 1e-4 bound, and the other fixed-order reductions."""
import numpy as np
import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import _lib, config as mgx_config, ops, schedule, sparse, tileplan

import exact_ladder as xl
from exact_ladder import assert_exact, assert_mean, exact_pair, ints, reduce_rows

DEV = "cuda:0"
WIDTHS = [1, 2, 4, 7, 16, 41, 64, 100, 128, 132, 256, 320]
GROUPS = (2, 4, 8, 16, 32, 64)


@pytest.fixture()
def cpu_on():
    was = mg.enable_cpu_backend(True)
    try:
        yield
    finally:
        mg.enable_cpu_backend(was)


_graphs = {}


def ladder(bipartite=False, **kw):
    key = (bipartite, tuple(sorted(kw.items())))
    if key not in _graphs:
        _graphs[key] = xl.ladder_graph(seed=int(bipartite), bipartite=bipartite, **{k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()})
    return _graphs[key]


_refs = {}


def memo(G, what, make):
    """References are a function of (graph, case) alone: built once per session, shared by every schedule, id width and backend."""
    key = (id(G[0]), what)
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def T(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)       # a copy also on the host: kernels write into some of these


def N(t):
    return t.detach().cpu().numpy()


def make_csr(G, idtype, dev):
    src, dst, n_src, n_dst = G
    return sparse.coo_to_csr(n_dst, n_src, torch.from_numpy(dst).to(idtype).to(dev), torch.from_numpy(src).to(idtype).to(dev))


def view_of(csr, kind="none", split=256, seed=1):
    """A view of `csr` with the schedule fixed by the test: no plan, natural order or a shuffled row order, hubs split at `split`;
    never the tile kernel, never the lane-group kernel (their tests force them themselves)."""
    v = sparse.CsrView(csr.num_rows, csr.num_cols, csr.indptr, csr.indices, csr.eids)
    v._plan, v._tile_plan = None, None
    v._short = {nb: None for nb in GROUPS}
    if kind != "none" and csr.indptr.is_cuda:
        order = None
        if kind == "shuffled":
            order = torch.randperm(csr.num_rows, generator=torch.Generator().manual_seed(seed)).to(csr.device)
        v._plan = schedule.build_plan(v, order, split, "natural" if order is None else "cluster")
        assert v._plan.num_hubs >= 1 and v._plan.num_slots >= 2 * v._plan.num_hubs
    return v


def last_kernel():
    return _lib.lib().mgx_last_spmm_kernel().decode()


def degrees(G):
    return np.bincount(G[1], minlength=G[3])


# ============================================================================= the cases, shared by the CPU and the GPU tests
def copy_u_cases(views, G, dev, widths, kernels=None, extras=True):
    src, dst, n_src, n_dst = G
    deg = degrees(G)
    for D in widths:
        def make(D=D):
            rng = np.random.default_rng(100 + D)
            X = ints(rng, (n_src, D), 8)
            want, mag = exact_pair(dst, n_dst, lambda c: X[:, c][src], D, with_mag=True)
            ss, ds, base = ints(rng, n_src, 2), ints(rng, n_dst, 3), ints(rng, (n_dst, D), 8)
            Xs = X * ss[:, None]                  # |ss| <= 2, |ds| <= 3, |base| <= 8: the sum of |terms| is at most 8 + 3 * 2 * mag
            assert 8 + 6 * int(mag.max()) < xl.LIMIT
            want_acc = base.astype(np.int64) + ds.astype(np.int64)[:, None] * reduce_rows(dst, n_dst, lambda c: Xs[:, c][src], D)
            return X, want, ss, ds, base, want_acc
        X, want, ss, ds, base, want_acc = memo(G, ("copy_u", D), make)
        x = T(X, dev)
        for name, v in views:
            what = "copy_u D=%d %s" % (D, name)
            out = sparse.gspmm_raw(v, "copy_lhs", "sum", x, None, dense_out=True)[0]
            if kernels is not None:
                assert last_kernel() in kernels, (what, last_kernel())
            assert_exact(N(out), want, what + " sum")
            assert_mean(N(sparse.gspmm_raw(v, "copy_lhs", "mean", x, None, dense_out=True)[0]), want, deg, what + " mean")
            if extras:
                acc = T(base, dev)
                sparse.gspmm_raw(v, "copy_lhs", "sum", x, None, src_scale=T(ss, dev), dst_scale=T(ds, dev), accumulate_into=acc)
                assert_exact(N(acc), want_acc, what + " accumulate + scales")


def edge_operand_cases(views, G, dev, kernels=None, parts=("copy_e", "mul", "add", "add mean")):
    """copy_e, u_mul_e (scalar, per-head and full-width weights) and u_add_e (two launches, the second accumulating, two hub fix-ups)."""
    src, dst, n_src, n_dst = G
    nnz = src.shape[0]
    deg = degrees(G)

    def run(op, red, xs, es, want, what):
        for name, v in views:
            out = sparse.gspmm_raw(v, op, red, None if xs is None else T(xs, dev), None if es is None else T(es, dev), dense_out=True)[0]
            if kernels is not None:
                assert last_kernel() in kernels, (what, name, last_kernel())
            got = N(out).reshape(n_dst, -1)
            if red == "sum":
                assert_exact(got, want, "%s %s" % (what, name))
            else:
                assert_mean(got, want, deg, "%s %s" % (what, name))

    for D in (1, 4, 41, 64, 132) if "copy_e" in parts else ():
        def make(D=D):
            E = ints(np.random.default_rng(700 + D), (nnz, D), 8)
            return E, exact_pair(dst, n_dst, lambda c: E[:, c], D)
        E, want = memo(G, ("copy_e", D), make)
        run("copy_rhs", "sum", None, E, want, "copy_e D=%d" % D)
        run("copy_rhs", "mean", None, E, want, "copy_e mean D=%d" % D)
    # scalar weights over VEC 1 / ragged / 4 / two passes, per-head weights H = 3, 8 (and H = 1 as the scalar), full-width weights (F = 1)
    for H, F in [(1, 1), (1, 7), (1, 64), (1, 132), (1, 320), (3, 4), (3, 5), (8, 8), (41, 1), (64, 1)] if "mul" in parts else ():
        D = H * F

        def make(H=H, F=F, D=D):
            rng = np.random.default_rng(800 + 10 * D + H)
            X, W = ints(rng, (n_src, H, F), 8), ints(rng, (nnz, H, 1), 4)
            X2 = X.reshape(n_src, D)
            return X, W, exact_pair(dst, n_dst, lambda c: X2[:, c][src] * W[:, np.arange(c.start, c.stop) // F, 0], D)
        X, W, want = memo(G, ("mul", H, F), make)
        if H == 1:
            run("mul", "sum", X.reshape(n_src, D), W.reshape(nnz, 1), want, "u_mul_e scalar D=%d" % D)
        else:
            run("mul", "sum", X, W, want, "u_mul_e H=%d F=%d" % (H, F))
        run("mul", "mean", X, W, want, "u_mul_e mean H=%d F=%d" % (H, F))
    for D in (1, 4, 41, 64, 100, 132, 256) if "add" in parts or "add mean" in parts else ():
        def make(D=D):
            rng = np.random.default_rng(900 + D)
            X, E = ints(rng, (n_src, D), 8), ints(rng, (nnz, D), 8)
            return X, E, exact_pair(dst, n_dst, lambda c: X[:, c][src] + E[:, c], D)
        X, E, want = memo(G, ("add", D), make)
        if "add" in parts:
            run("add", "sum", X, E, want, "u_add_e D=%d" % D)
        if "add mean" in parts:
            run("add", "mean", X, E, want, "u_add_e mean D=%d" % D)


def select_reference(dst, n_dst, term, red):
    """(values, winning edge id) of max | min per (row, column); term [nnz, K] integers without ties inside a row; empty rows: 0, -1."""
    K = term.shape[1]
    counts = np.bincount(dst, minlength=n_dst)
    starts = np.cumsum(counts) - counts
    live = counts > 0
    val, arg = np.zeros((n_dst, K), np.int64), np.full((n_dst, K), -1, np.int64)
    for k in range(K):
        order = np.lexsort((term[:, k], dst))
        pick = (starts + counts - 1)[live] if red == "max" else starts[live]
        arg[live, k] = order[pick]
        val[live, k] = term[order[pick], k]
        srt = term[order, k]
        same = (srt[1:] == srt[:-1]) & (dst[order][1:] == dst[order][:-1])
        assert not same.any(), "the test's own terms tie inside a row"
    return val, arg


def max_min_cases(view, G, dev, kernel=None):
    """u_add_e max / min through a broadcast offset table ((N, 1, F) + (E, H, 1)), distinct terms per row: head 0 all negative, head 1
    all positive -- a wrong identity element shows; and copy_u with distinct source values."""
    src, dst, n_src, n_dst = G
    nnz = src.shape[0]
    rng = np.random.default_rng(3)
    H, F = 2, 3
    top = int(degrees(G).max())
    U = rng.integers(0, 2, (n_src, 1, F)).astype(np.float32)
    rank = np.stack([xl.rank_in_row(dst, rng.permutation(nnz)) for _ in range(H)], 1)
    E = (2 * rank + np.array([-(2 * top + 10), 10])[None, :]).astype(np.float32).reshape(nnz, H, 1)
    term = (U[src] + E).reshape(nnz, H * F).astype(np.int64)
    assert int(np.abs(term).max()) < xl.LIMIT and bool((term[:, :F] < 0).all()) and bool((term[:, F:] > 0).all())
    idt = view.indptr.dtype
    for red in ("max", "min"):
        val, arg = select_reference(dst, n_dst, term, red)
        out, au, ae = sparse.gspmm_raw(view, "add", red, T(U, dev), T(E, dev), want_arg=True)
        if kernel is not None:
            assert last_kernel() == kernel
        assert au.dtype == idt and ae.dtype == idt
        assert_exact(N(out).reshape(n_dst, -1), val, "u_add_e " + red)
        assert np.array_equal(N(ae).reshape(n_dst, -1), arg), "arg_e " + red
        assert np.array_equal(N(au).reshape(n_dst, -1), np.where(arg >= 0, src[np.maximum(arg, 0)], -1)), "arg_u " + red
        assert not N(out)[degrees(G) == 0].any()
    for shift in (-(n_src + 5), 5):             # every value negative / positive
        X = np.stack([rng.permutation(n_src) + shift for _ in range(4)], 1).astype(np.float32)
        for red in ("max", "min"):
            # (ties between parallel edges of one source are the same value AND the same arg)
            out, au, _ = sparse.gspmm_raw(view, "copy_lhs", red, T(X, dev), None, want_arg=True)
            if kernel is not None:
                assert last_kernel() == kernel
            want = np.zeros((n_dst, 4), np.int64)
            want_u = np.full((n_dst, 4), -1, np.int64)
            for k in range(4):
                m = np.full(n_dst, np.iinfo(np.int64).min if red == "max" else np.iinfo(np.int64).max)
                (np.maximum if red == "max" else np.minimum).at(m, dst, X[src, k].astype(np.int64))
                live = degrees(G) > 0
                want[live, k] = m[live]
                where = np.full(n_src + 2 * abs(shift) + 1, -1, np.int64)
                where[X[:, k].astype(np.int64) - min(shift, 0)] = np.arange(n_src)
                want_u[live, k] = where[m[live] - min(shift, 0)]
            assert_exact(N(out), want, "copy_u %s shift %d" % (red, shift))
            assert np.array_equal(N(au), want_u), "copy_u arg %s" % red


def graph_of(G, idtype, dev):
    src, dst, n_src, n_dst = G
    if n_src == n_dst:
        g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n_src)
        g = g.int() if idtype == torch.int32 else g.long()
        return g.to(dev)
    return mg.create_block((torch.from_numpy(src), torch.from_numpy(dst)), n_src, n_dst, idtype=idtype, device=dev)


def autograd_cases(G, g, dev):
    """ops.gspmm(copy_lhs | mul, sum) backward with an integer upstream gradient: X.grad is the int64 transpose product, E.grad the
    exact per-edge dot."""
    src, dst, n_src, n_dst = G
    nnz = src.shape[0]
    rng = np.random.default_rng(11)
    for H, F in ((1, 64), (1, 41), (3, 4), (8, 8)):
        D = H * F
        X, W, dZ = ints(rng, (n_src, H, F), 8), ints(rng, (nnz, H, 1), 4), ints(rng, (n_dst, H, F), 8)
        dZ2 = dZ.reshape(n_dst, D)
        x = T(X, dev).requires_grad_(True)
        ops.gspmm(g, "copy_lhs", "sum", x, None).backward(T(dZ, dev))
        assert_exact(N(x.grad).reshape(n_src, D), exact_pair(src, n_src, lambda c: dZ2[:, c][dst], D), "copy_u X.grad H=%d F=%d" % (H, F))
        x = T(X, dev).requires_grad_(True)
        w = T(W, dev).requires_grad_(True)
        ops.gspmm(g, "mul", "sum", x, w).backward(T(dZ, dev))
        want_x = exact_pair(src, n_src, lambda c: dZ2[:, c][dst] * W[:, np.arange(c.start, c.stop) // F, 0], D)
        assert_exact(N(x.grad).reshape(n_src, D), want_x, "u_mul_e X.grad H=%d F=%d" % (H, F))
        dot = (X[src].astype(np.int64) * dZ[dst].astype(np.int64)).sum(-1, keepdims=True)
        assert int((np.abs(X[src]).astype(np.int64) * np.abs(dZ[dst]).astype(np.int64)).sum(-1).max()) < xl.LIMIT
        assert_exact(N(w.grad), dot, "u_mul_e E.grad H=%d F=%d" % (H, F))


def row_constants(n_dst):
    c = ((np.arange(n_dst) * 37) % 161 - 80).astype(np.float32)
    assert c.min() == -80 and c.max() == 80
    return c


def softmax_uniform_case(be, view, G, H, dev):
    """z constant inside a row (another constant per row and head, +-80 included): expf(0) = 1 and the sum deg are exact, so
    a == 1 / deg within 1 ulp -- a chunk lost or counted twice changes deg."""
    src, dst, n_src, n_dst = G
    deg = degrees(G)
    c = row_constants(n_dst)
    sign = np.where(np.arange(H) % 2 == 0, 1.0, -1.0).astype(np.float32)
    z = c[dst][:, None] * sign[None, :]
    want = (np.float32(1) / deg[dst].astype(np.float32))[:, None].repeat(H, 1)
    a = N(be.edge_softmax_fwd(view, T(z, dev)))
    assert bool(xl.within_ulp(a, want, 1).all()), ("edge_softmax uniform", H, float(np.abs(a - want).max()))
    # the fused form: el the same for every source, er the row constant; negative sums take the leaky branch (slope 0.25: exact)
    el = np.repeat((np.arange(H) % 3 - 1).astype(np.float32)[None, :], n_src, 0) * 4
    er = (c[:, None] * sign[None, :]).astype(np.float32) * 4
    a = N(be.gat_attention_fwd(view, T(el, dev), T(er, dev), 0.25))
    assert bool(xl.within_ulp(a, want, 1).all()), ("gat_attention uniform", H, float(np.abs(a - want).max()))


def softmax_register_cache():
    """kCache of csrc/softmax.hip: a row is held in registers while in-degree * LH <= 64 * kCache."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(sparse.__file__)), "..", "csrc", "softmax.hip")).read()
    found = re.search(r"constexpr\s+int\s+kCache\s*=\s*(\d+)\s*;", text)
    assert found, "csrc/softmax.hip no longer declares kCache: the register / re-read boundary below is not probed"
    return int(found.group(1))


def hot_positions(lens, H, split, rnd):
    """Position of the hot edge inside every non-empty row, per head: first, last, 63 / 64 / 65, around the register-cache limit
    kCache * 64 / LH of csrc/softmax.hip, around the first, second and last chunk boundary of a split row and around eight more
    boundaries k * split spaced evenly over the row, cycling with the row, the head and `rnd`."""
    LH = 1
    while LH < H:
        LH *= 2
    cache = softmax_register_cache() * 64 // LH
    pos = np.zeros((lens.shape[0], H), np.int64)
    for v, L in enumerate(lens.tolist()):
        if L == 0:
            continue
        cand = [0, L - 1, 63, 64, 65, cache - 1, cache, cache + 1, split - 1, split, split + 1, 2 * split - 1, 2 * split,
                (L - 1) // split * split, (L - 1) // split * split - 1, L // 2]
        chunks = (L - 1) // split
        for k in sorted({(chunks * i) // 9 for i in range(1, 9)} - {0}):
            cand += [k * split - 1, k * split]
        cand = sorted({p for p in cand if 0 <= p < L})
        for h in range(H):
            pos[v, h] = cand[(v + h + rnd) % len(cand)]
    return pos


def softmax_one_hot_case(be, G, H, dev, idtype, make_view, split, rounds):
    """One edge per row at z = 200, the rest at 0 (expf(-200) == 0 in fp32): a is exactly 1 there and exactly 0 elsewhere.  The fused
    form gets the same logits from el = 200 on a source that only the hot edges read."""
    assert np.exp(np.float32(-200)) == 0
    src, dst, n_src, n_dst = G
    nnz = src.shape[0]
    lens = degrees(G)
    order = np.argsort(dst, kind="stable")          # CSR position -> edge id (the CSR build is stable)
    starts = np.cumsum(lens) - lens
    live = np.nonzero(lens > 0)[0]
    view = make_view(make_csr(G, idtype, dev))
    assert np.array_equal(N(view.eids), order)
    cols = torch.arange(H, device=dev)
    for rnd in rounds:
        pos = hot_positions(lens, H, split, rnd)
        hot = order[(starts[:, None] + pos)[live]]                      # [live rows, H] edge ids
        want = torch.zeros((nnz, H), device=dev)
        want[T(hot, dev), cols] = 1.0
        a = be.edge_softmax_fwd(view, want * 200.0)
        assert torch.equal(a, want), ("edge_softmax one-hot", H, rnd, int((a != want).sum()))
    # fused: source 0 carries el = 200 and is read by the hot edge of every row alone (head 0's position); every other source a
    # non-positive multiple of 4 (leaky branch, slope 0.25), er a small row constant
    rng = np.random.default_rng(5)
    for rnd in list(rounds)[:3]:
        pos = hot_positions(lens, 1, split, rnd)[:, 0]
        src2 = np.where(src == 0, 1, src)
        hot = order[(starts + pos)[live]]
        src2[hot] = 0
        G2 = (src2, dst, n_src, n_dst)
        view2 = make_view(make_csr(G2, idtype, dev))
        el = -4.0 * rng.integers(0, 4, (n_src, H)).astype(np.float32)
        el[0] = 200.0
        er = rng.integers(-3, 4, (n_dst, H)).astype(np.float32)
        z = el[src2] + er[dst]
        z = np.where(z > 0, z, np.float32(0.25) * z)
        cold = np.ones(nnz, bool)
        cold[hot] = False
        gap = float(z[hot].min() - z[cold].max())                      # hot 200 + er against at most 0 + er <= 3 in its row
        assert gap >= 190 and np.exp(np.float32(-gap)) == 0, gap
        want = np.zeros((nnz, H), np.float32)
        want[hot] = 1.0
        a = N(be.gat_attention_fwd(view2, T(el, dev), T(er, dev), 0.25))
        assert np.array_equal(a, want), ("gat_attention one-hot", H, rnd, int((a != want).sum()))


# ============================================================================= CPU: helpers, plan builders, the OpenMP variants
def test_ladder_has_every_rung_and_the_promised_shape():
    for bip in (False, True):
        src, dst, n_src, n_dst = ladder(bip)
        lens = degrees((src, dst, n_src, n_dst))
        have = set(lens.tolist())
        want = set(xl.BASE_LENGTHS) | {xl.LONGEST}
        for S in {mgx_config.HUB_SPLIT, 64, 1024, mgx_config.TILE_HUB_SPLIT}:
            want |= set(xl.around(S))
        assert want <= have and lens.max() == xl.LONGEST and int((lens == xl.LONGEST).sum()) == 1
        assert n_dst > xl.min_rows() > 64 and (n_src != n_dst) == bip
        top = max(mgx_config.HUB_SPLIT, mgx_config.TILE_HUB_SPLIT, 1024)
        assert lens[0] > top and lens[1] > top and lens[-1] > top            # hub rows first, adjacent and last
        per_src = np.bincount(src, minlength=n_src)
        assert per_src.max() >= 3000 and int((per_src == 0).sum()) >= 40      # a hub source; sources nobody gathers
        pairs = np.unique(dst * n_src + src)
        assert pairs.shape[0] < src.shape[0] and bool((np.diff(dst) < 0).any())   # a multigraph in a shuffled edge order
        assert np.array_equal(xl.ladder_graph(seed=0, bipartite=bip)[0], xl.ladder_graph(seed=0, bipartite=bip)[0])


def test_reduce_rows_is_np_add_at():
    src, dst, n_src, n_dst = ladder()
    X = ints(np.random.default_rng(0), (n_src, 70), 8).astype(np.int64)
    ref = np.zeros((n_dst, 70), np.int64)
    np.add.at(ref, dst, X[src])
    assert np.array_equal(reduce_rows(dst, n_dst, lambda c: X[:, c][src], 70), ref)
    mag = np.zeros((n_dst, 70), np.int64)
    np.add.at(mag, dst, np.abs(X[src]))
    assert np.array_equal(reduce_rows(dst, n_dst, lambda c: X[:, c][src], 70, absolute=True), mag)
    with pytest.raises(AssertionError):
        exact_pair(dst, n_dst, lambda c: 1000 * X[:, c][src], 70)              # 21 000 x 8 000 is past 2^24: refused


def test_comparator_self_test_old_metric_accepts_what_the_exact_one_rejects(oracle):
    """Why this module exists: one edge of the 21 000-edge row lost (or doubled).  The earlier metric -- |got - want| / (|want| + 1e-5)
    < 1e-4 against the fp32 oracle on U[0, 1) inputs -- accepts the damaged result; the exact comparison rejects it."""
    src, dst, n_src, n_dst = ladder()
    hub = 0
    assert degrees((src, dst, n_src, n_dst))[hub] == xl.LONGEST
    D = 4
    rng = np.random.default_rng(1)
    Xu = rng.random((n_src, D), dtype=np.float32)
    ip, ix, ei = oracle.coo_to_csr(n_dst, dst, src)
    fp32 = oracle.spmm(ip, ix, ei, "copy_lhs", "sum", Xu, None)
    in_hub = np.nonzero(dst == hub)[0]
    mid = ((Xu[src[in_hub]] > 0.25) & (Xu[src[in_hub]] < 0.75)).all(1)
    victim = int(in_hub[np.nonzero(mid)[0][0]])                                 # an ordinary edge: every term between 0.25 and 0.75
    for sign in (-1.0, 1.0):                                                    # lost / doubled: the oracle's own sums without / with it twice
        damaged = fp32.copy()
        damaged[hub] += np.float32(sign) * Xu[src[victim]]
        assert not np.array_equal(damaged, fp32)
        assert xl.old_metric(damaged, fp32) < 1e-4
        assert xl.old_metric(damaged[hub] / np.float32(xl.LONGEST), fp32[hub] / np.float32(xl.LONGEST)) < 1e-4
    Xi = ints(rng, (n_src, D), 8)
    Xi[src[victim]] = [1, -1, 1, 1]                                             # an edge of value 1 (magnitude)
    want = exact_pair(dst, n_dst, lambda c: Xi[:, c][src], D)
    assert_exact(want.astype(np.float32), want)
    for keep in (np.arange(src.shape[0]) != victim, None):
        s2, d2 = (src[keep], dst[keep]) if keep is not None else (np.append(src, src[victim]), np.append(dst, hub))
        damaged = reduce_rows(d2, n_dst, lambda c: Xi[:, c][s2], D)
        assert int(np.abs(damaged - want).sum()) == D and int(np.abs(damaged - want).max()) == 1
        with pytest.raises(AssertionError):
            assert_exact(damaged.astype(np.float32), want)
        with pytest.raises(AssertionError):
            assert_mean(xl.mean_of(damaged, np.bincount(dst, minlength=n_dst)), want, np.bincount(dst, minlength=n_dst))
    deg = np.bincount(dst, minlength=n_dst)
    assert_mean(xl.mean_of(want, deg), want, deg)
    assert_mean((want.astype(np.float32) * (np.float32(1) / np.maximum(deg, 1).astype(np.float32))[:, None]), want, deg)   # reciprocal + multiply


def walk_plan(plan, csr, X):
    """The row kernels' walk of a schedule on the host in int64: direct items write their row, chunks their partial slot, the fix-up
    adds a hub's slots.  Also checks that the items tile every row exactly once."""
    ip = N(csr.indptr.long())
    n = csr.num_rows
    cs = np.concatenate([np.zeros((1, X.shape[1]), np.int64), np.cumsum(X[N(csr.indices.long())].astype(np.int64), 0)])
    row, beg, end = N(plan.item_row).astype(np.int64), N(plan.item_beg.long()), N(plan.item_end.long())
    node = N(plan.item_node).astype(np.int64)
    sums = cs[end] - cs[beg]
    out = np.zeros((n, X.shape[1]), np.int64)
    direct = row >= 0
    assert np.array_equal(np.sort(np.concatenate([row[direct], N(plan.hub_row)])), np.arange(n))
    assert np.array_equal(beg[direct], ip[row[direct]]) and np.array_equal(end[direct], ip[row[direct] + 1]) and np.array_equal(node[direct], row[direct])
    out[row[direct]] = sums[direct]
    partial = np.zeros((max(plan.num_slots, 1), X.shape[1]), np.int64)
    slots = -(row[~direct] + 1)
    assert np.array_equal(np.sort(slots), np.arange(plan.num_slots)) and np.array_equal(N(plan.slot_item)[slots], np.nonzero(~direct)[0])
    partial[slots] = sums[~direct]
    hub_row, ptr = N(plan.hub_row), N(plan.hub_slot_ptr)
    covered = np.zeros(n, np.int64)
    np.add.at(covered, node[~direct], (end - beg)[~direct])
    for h in range(plan.num_hubs):
        out[hub_row[h]] = partial[ptr[h]:ptr[h + 1]].sum(0)
        assert covered[hub_row[h]] == ip[hub_row[h] + 1] - ip[hub_row[h]]
    return out


def test_plan_builder_on_the_ladder():
    """schedule.build_plan on host tensors (the torch builder, whatever config.PLAN_BUILDER says); the device builder is compared with
    it in test_device_plan_builder_equals_the_torch_builder."""
    for bip in (False, True):
        G = ladder(bip)
        src, dst, n_src, n_dst = G
        csr = make_csr(G, torch.int32, "cpu")
        X = ints(np.random.default_rng(2), (n_src, 3), 8)
        want = exact_pair(dst, n_dst, lambda c: X[:, c][src], 3)
        for split in xl.split_thresholds():
            for order in (None, torch.randperm(n_dst, generator=torch.Generator().manual_seed(split))):
                plan = schedule.build_plan(csr, order, split, "natural")
                lens = degrees(G)
                assert plan.num_hubs == int((lens > split).sum()) and plan.num_slots == int((-(-lens[lens > split] // split)).sum())
                assert int((plan.item_end - plan.item_beg).max()) <= split
                assert np.array_equal(walk_plan(plan, csr, X), want), split


@pytest.mark.parametrize("lanes_log2", [4, 3, 2])
def test_tile_plans_of_the_ladder_walk_to_the_exact_product(lanes_log2):
    G = ladder(True)
    src, dst, n_src, n_dst = G
    csr = make_csr(G, torch.int32, "cpu")
    X = ints(np.random.default_rng(4), (n_src, 2), 8)
    want = exact_pair(dst, n_dst, lambda c: X[:, c][src], 2)
    for split, order in ((mgx_config.TILE_HUB_SPLIT, torch.randperm(n_dst, generator=torch.Generator().manual_seed(3))), (64, None)):
        base = schedule.build_plan(csr, order, split, "cluster")
        tp = tileplan.build_tile_plan(csr, base, *mgx_config.TILE_CONFIG[lanes_log2], lanes_log2=lanes_log2)
        assert tileplan.validate(tp, csr) and tp.num_tiles >= 2
        out, part = tileplan.emulate(tp, torch.from_numpy(X), n_dst, base.num_slots)
        hub_row, ptr = base.hub_row.numpy(), base.hub_slot_ptr.numpy()
        for h in range(base.num_hubs):
            out[hub_row[h]] += part[ptr[h]:ptr[h + 1]].sum(0)
        assert np.array_equal(out, want.astype(np.float64)), (lanes_log2, split)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bipartite", [False, True])
def test_cpu_variants_sum_family(cpu_on, idtype, bipartite):
    G = ladder(bipartite)
    views = [("cpu", view_of(make_csr(G, idtype, "cpu")))]
    copy_u_cases(views, G, "cpu", WIDTHS if idtype == torch.int32 and not bipartite else [1, 7, 64, 132])
    if idtype == torch.int32 and bipartite:
        edge_operand_cases(views, G, "cpu")


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_cpu_variants_max_min_with_args(cpu_on, idtype):
    G = ladder(True)
    max_min_cases(view_of(make_csr(G, idtype, "cpu")), G, "cpu")


def test_cpu_variants_autograd(cpu_on):
    G = ladder(True)
    autograd_cases(G, graph_of(G, torch.int32, "cpu"), "cpu")


@pytest.mark.parametrize("H", [1, 3, 8, 64])
def test_cpu_variants_softmax_uniform_and_one_hot(cpu_on, H):
    G = ladder(False)
    be = sparse.backend_for(torch.zeros(1))
    softmax_uniform_case(be, view_of(make_csr(G, torch.int32, "cpu")), G, H, "cpu")
    softmax_one_hot_case(be, G, H, "cpu", torch.int32, view_of, 256, rounds=range(2))


# ============================================================================= GPU: the g-SpMM families
def gpu_views(csr, splits=(64, 256, 1024)):
    views = [("no plan", view_of(csr))]
    for s in splits:
        views.append(("natural/%d" % s, view_of(csr, "natural", s)))
    views.append(("shuffled/256", view_of(csr, "shuffled", 256)))
    views.append(("shuffled/64", view_of(csr, "shuffled", 64, seed=2)))
    return views


@pytest.mark.gpu
@pytest.mark.parametrize("bipartite", [False, True])
def test_row_kernels_copy_u_every_width_and_schedule(bipartite):
    G = ladder(bipartite)
    copy_u_cases(gpu_views(make_csr(G, torch.int32, DEV)), G, DEV, WIDTHS, kernels=("rowwave32",))


@pytest.mark.gpu
def test_row_kernels_int64_ids_take_the_non_lean_kernels():
    G = ladder(True)
    seen = set()
    csr = make_csr(G, torch.int64, DEV)
    views = [("no plan", view_of(csr)), ("natural/256", view_of(csr, "natural", 256)), ("shuffled/64", view_of(csr, "shuffled", 64))]
    for D in WIDTHS:
        copy_u_cases(views, G, DEV, [D], kernels=("fast", "rowwave"), extras=D in (4, 41, 128))
        seen.add(last_kernel())
    edge_operand_cases(views[1:2], G, DEV, kernels=("fast", "rowwave"), parts=("copy_e", "mul", "add"))
    assert seen == {"rowwave"}                                  # ~970 edges per row: a wave per item at every width
    # rows short enough that the 64-bit path gives every lane group a row of its own (spmm_fast_kernel): the rungs up to 65
    short = ladder(True, base=tuple(b for b in xl.BASE_LENGTHS if b <= 65), thresholds=(16,), longest=0, repeats=8, hub_source_edges=300)
    csr = make_csr(short, torch.int64, DEV)
    seen = set()
    for D in (1, 2, 4, 7, 16, 41, 64, 128):
        copy_u_cases([("no plan", view_of(csr)), ("natural/16", view_of(csr, "natural", 16))], short, DEV, [D], kernels=("fast", "rowwave"))
        seen.add(last_kernel())
    assert seen == {"fast", "rowwave"}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_device_plan_builder_equals_the_torch_builder(idtype, monkeypatch):
    """mgx_spmm_plan_count / _fill (csrc/plan.hip) on the ladder: the tables of the torch builder, and their walk is the exact product."""
    G = ladder(True)
    src, dst, n_src, n_dst = G
    csr = make_csr(G, idtype, DEV)
    X = ints(np.random.default_rng(2), (n_src, 3), 8)
    want = exact_pair(dst, n_dst, lambda c: X[:, c][src], 3)
    for split in xl.split_thresholds():
        for order in (None, torch.randperm(n_dst, generator=torch.Generator().manual_seed(split)).to(DEV)):
            plans = {}
            for builder in ("device", "torch"):
                monkeypatch.setattr(mgx_config, "PLAN_BUILDER", builder)
                plans[builder] = schedule.build_plan(csr, order, split, "natural")
            a, b = plans["device"], plans["torch"]
            assert a.num_slots == b.num_slots and a.num_hubs == b.num_hubs
            for name in ("item_row", "item_beg", "item_end", "item_node", "hub_row", "hub_slot_ptr", "slot_item"):
                assert torch.equal(getattr(a, name).long(), getattr(b, name).long()), (name, split)
            assert np.array_equal(walk_plan(a, csr, X), want), split


@pytest.mark.gpu
def test_row_kernels_edge_operands():
    G = ladder(False)
    csr = make_csr(G, torch.int32, DEV)
    views = [("no plan", view_of(csr)), ("natural/64", view_of(csr, "natural", 64)), ("shuffled/256", view_of(csr, "shuffled", 256)),
             ("natural/1024", view_of(csr, "natural", 1024))]
    edge_operand_cases(views, G, DEV, kernels=("rowwave32",), parts=("copy_e", "mul", "add"))


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_u_add_e_mean_is_an_exact_sum_and_one_division(idtype):
    """u_add_e / mean with full-width operands runs as two launches (csrc/spmm.hip, spmm_impl): copy_u, then copy_e accumulating.  Both
    leave unscaled sums and spmm_row_scale_kernel divides the exact total once.  The earlier form, mean(U) + mean(E), rounded two
    quotients: where the two sums cancel it was 7 ulp off on the ladder graph (row 85, D = 1: 0.002766475 for 0.0027664767), inside
    the 1e-4 x sum-of-|terms| bound of the rest of the suite and outside the 4-ulp rule for `mean`."""
    G = ladder(False)
    csr = make_csr(G, idtype, DEV)
    views = [("no plan", view_of(csr)), ("natural/256", view_of(csr, "natural", 256))]
    edge_operand_cases(views, G, DEV, kernels=("rowwave32",) if idtype == torch.int32 else ("fast", "rowwave"), parts=("add mean",))


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [32, 16, 5])
def test_two_part_plans_write_every_row_exactly_once(limit):
    """MGX_SPMM_SHORT_ROWS with a `rest` part: rows of 31, 32, 33 edges decide which part owns a row.  NaN-filled outputs: a row nobody
    writes stays NaN; accumulate: a row written twice is doubled."""
    G = ladder(True)
    src, dst, n_src, n_dst = G
    deg = degrees(G)
    csr = make_csr(G, torch.int32, DEV)
    be = sparse.backend_for(csr.indptr)
    for kind, split in (("natural", 256), ("shuffled", 64)):
        v = view_of(csr, kind, split)
        plan = schedule.split_short_items(v, v.plan(), any_share=True, limit=limit)[0]
        assert plan.rest is not None and plan.rest.num_slots >= 8
        assert int((plan.item_end - plan.item_beg).max()) == limit      # 32 | 16 | 5: ladder rungs, as are 33 and 17 on the other side
        assert int((plan.rest.item_end - plan.rest.item_beg)[plan.rest.item_row >= 0].min()) == {32: 33, 16: 17, 5: 7}[limit]
        v._short = {nb: plan for nb in GROUPS}
        rng = np.random.default_rng(limit)
        for D in (4, 16, 32, 64, 100, 128):
            X = ints(rng, (n_src, D), 8)
            want = exact_pair(dst, n_dst, lambda c: X[:, c][src], D)
            x = T(X, DEV)
            for red in ("sum", "mean"):
                out = torch.full((n_dst, D), float("nan"), device=DEV)
                be.spmm_copy_u_strided(v, red, x, out)
                assert last_kernel() == "rowgroup32", (D, last_kernel())
                (assert_exact if red == "sum" else lambda g_, w_, m_: assert_mean(g_, w_, deg, m_))(N(out), want, "two-part D=%d %s" % (D, red))
            base, ds = ints(rng, (n_dst, D), 8), ints(rng, n_dst, 3)
            assert int((np.abs(base) + np.abs(ds)[:, None] * reduce_rows(dst, n_dst, lambda c: X[:, c][src], D, absolute=True)).max()) < xl.LIMIT
            acc = T(base, DEV)
            sparse.gspmm_raw(v, "copy_lhs", "sum", x, None, dst_scale=T(ds, DEV), accumulate_into=acc)
            assert last_kernel() == "rowgroup32"
            assert_exact(N(acc), base.astype(np.int64) + ds.astype(np.int64)[:, None] * want, "two-part accumulate D=%d" % D)
            if D <= 32:
                E = ints(rng, (src.shape[0], D), 8)
                out = sparse.gspmm_raw(v, "copy_rhs", "sum", None, T(E, DEV))[0]
                assert last_kernel() == "rowgroup32"
                assert_exact(N(out), exact_pair(dst, n_dst, lambda c: E[:, c], D), "two-part copy_e D=%d" % D)


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_generic_kernel_max_min_with_args_and_an_offset_table(idtype):
    G = ladder(True)
    max_min_cases(view_of(make_csr(G, idtype, DEV)), G, DEV, kernel="generic")


@pytest.mark.gpu
def test_masked_kernel_treats_minus_zero_rows_as_zero_rows():
    G = ladder(True)
    src, dst, n_src, n_dst = G
    deg = degrees(G)
    csr = make_csr(G, torch.int32, DEV)
    be = sparse.backend_for(csr.indptr)
    rng = np.random.default_rng(8)
    for D in (4, 64, 100):
        X = ints(rng, (n_src, D), 8)
        X[rng.random(n_src) < 0.5] = 0.0
        X[np.arange(5, n_src, 7)] = -0.0                       # a row of -0.0 is a zero row
        X[3] = 0.0                                              # the hub source: one non-zero, in the last column
        X[3, D - 1] = 5.0
        X[np.arange(6, n_src, 11), :] = 0.0
        X[np.arange(6, n_src, 11), D - 1] = -1.0
        x = T(X, DEV)
        bits = be.row_nonzero_bits(x)
        live = (X != 0).any(1)
        assert bool(np.signbit(X[5]).all()) and not live[5] and live[3] and live[6]
        words = N(bits).view(np.uint32)
        got_bits = (words[np.arange(n_src) // 32] >> (np.arange(n_src) % 32).astype(np.uint32)) & 1
        assert np.array_equal(got_bits.astype(bool), live)
        want = exact_pair(dst, n_dst, lambda c: X[:, c][src], D)
        for name, v in gpu_views(csr, splits=(64, 256)):
            assert_exact(N(be.spmm_copy_u_masked(v, "sum", x, bits)), want, "masked D=%d %s" % (D, name))
            assert last_kernel() == "rowwave32"
            assert_mean(N(be.spmm_copy_u_masked(v, "mean", x, bits)), want, deg, "masked mean D=%d %s" % (D, name))
            base, ds = ints(rng, (n_dst, D), 8), ints(rng, n_dst, 3)
            acc = T(base, DEV)
            be.spmm_copy_u_masked(v, "sum", x, bits, dst_scale=T(ds, DEV), accumulate_into=acc)
            assert_exact(N(acc), base.astype(np.int64) + ds.astype(np.int64)[:, None] * want, "masked accumulate D=%d %s" % (D, name))


@pytest.mark.gpu
def test_strided_kernel_leaves_the_other_half_bitwise_unchanged():
    G = ladder(True)
    src, dst, n_src, n_dst = G
    deg = degrees(G)
    csr = make_csr(G, torch.int32, DEV)
    be = sparse.backend_for(csr.indptr)
    rng = np.random.default_rng(9)
    for D in (4, 64, 100, 128, 320):
        Xw = ints(rng, (n_src, 2 * D + 8), 8)
        X = np.ascontiguousarray(Xw[:, D:2 * D])
        want = exact_pair(dst, n_dst, lambda c: X[:, c][src], D)
        xw = T(Xw, DEV)
        for name, v in gpu_views(csr, splits=(64, 256)):
            for red in ("sum", "mean"):
                before = T(ints(rng, (n_dst, 3 * D), 8), DEV)
                before[0, 0], before[-1, -1] = float("nan"), float("-inf")
                wide = before.clone()
                be.spmm_copy_u_strided(v, red, xw[:, D:2 * D], wide[:, D:2 * D])
                assert last_kernel() == "rowwave32"
                got = N(wide[:, D:2 * D])
                (assert_exact if red == "sum" else lambda g_, w_, m_: assert_mean(g_, w_, deg, m_))(got, want, "strided D=%d %s %s" % (D, red, name))
                for part in (slice(0, D), slice(2 * D, 3 * D)):
                    assert torch.equal(wide[:, part].contiguous().view(torch.int32), before[:, part].contiguous().view(torch.int32))
            base, ds = ints(rng, (n_dst, 2 * D), 8), ints(rng, n_dst, 3)
            wide = T(base, DEV)
            be.spmm_copy_u_strided(v, "sum", xw[:, D:2 * D], wide[:, D:], accumulate=True, dst_scale=T(ds, DEV))
            assert_exact(N(wide[:, D:]), base[:, D:].astype(np.int64) + ds.astype(np.int64)[:, None] * want, "strided accumulate D=%d %s" % (D, name))
            assert torch.equal(wide[:, :D], T(base, DEV)[:, :D])


@pytest.mark.gpu
@pytest.mark.parametrize("lanes_log2", [4, 3, 2])
def test_tile_kernel_on_the_ladder(lanes_log2):
    """mgx_spmm_tile_copy_u in its three geometries with the project's TILE_CONFIG: base plans split at TILE_HUB_SPLIT and at 64 (most
    ladder rows become hubs), sum / mean / accumulate / strided."""
    cfg = mgx_config.TILE_CONFIG[lanes_log2]
    rng = np.random.default_rng(lanes_log2)
    for bip in (False, True):
        G = ladder(bip)
        src, dst, n_src, n_dst = G
        deg = degrees(G)
        csr = make_csr(G, torch.int32, DEV)
        be = sparse.backend_for(csr.indptr)
        plans = []
        for split, order in ((mgx_config.TILE_HUB_SPLIT, torch.randperm(n_dst, generator=torch.Generator().manual_seed(5)).to(DEV)), (64, None),
                             (mgx_config.TILE_HUB_SPLIT, None)):
            base = schedule.build_plan(csr, order, split, "cluster")
            assert base.num_hubs >= 1
            tp = tileplan.build_tile_plan(csr, base, *cfg, lanes_log2=lanes_log2)
            tileplan.validate(tp, csr)
            assert tp.num_tiles >= 2
            plans.append((split, tp))
        for D, stride in {4: ((64, 64), (128, 128), (100, 100), (64, 192)), 3: ((32, 32), (24, 24), (32, 96)),
                          2: ((16, 16), (8, 8), (4, 4), (12, 12), (16, 48))}[lanes_log2]:
            Xw = ints(rng, (n_src, stride), 8)
            X = np.ascontiguousarray(Xw[:, :D])
            want, mag = exact_pair(dst, n_dst, lambda c: X[:, c][src], D, with_mag=True)
            assert 8 + 3 * int(mag.max()) < xl.LIMIT                                  # |base| <= 8, |dst_scale| <= 3
            x = T(Xw, DEV)[:, :D]
            base_m, ds = ints(rng, (n_dst, 2 * D), 8), ints(rng, n_dst, 3)
            want_acc = base_m[:, D:].astype(np.int64) + ds.astype(np.int64)[:, None] * want
            for split, tp in plans:
                what = "tile lg=%d split=%d D=%d/%d" % (lanes_log2, split, D, stride)
                assert_exact(N(be.spmm_tile_copy_u(csr, tp, "sum", x)), want, what)
                assert last_kernel() == "tile"
                assert_mean(N(be.spmm_tile_copy_u(csr, tp, "mean", x)), want, deg, what + " mean")
                wide = T(base_m, DEV)
                be.spmm_tile_copy_u(csr, tp, "sum", x, out2d=wide[:, D:], accumulate=True, dst_scale=T(ds, DEV))
                assert_exact(N(wide[:, D:]), want_acc, what + " accumulate, strided")
                assert torch.equal(wide[:, :D], T(base_m, DEV)[:, :D])


@pytest.mark.gpu
def test_slot_kernel_at_the_24_value_boundary():
    """D = 64 operands with exactly 0, 1, 23, 24, 25 and 64 non-zeros per row (24 = kSlotValues), columns 0 and 63 among them, packed with
    a row factor: the aggregation against int64, the overflow rows' bytes against the slot format (csrc/slots.h)."""
    from test_spmm_slots import _reference_slots
    G = ladder(True)
    src, dst, n_src, n_dst = G
    deg = degrees(G)
    csr = make_csr(G, torch.int32, DEV)
    be = sparse.backend_for(csr.indptr)
    rng = np.random.default_rng(10)
    counts = np.array([0, 1, 23, 24, 25, 64])[np.arange(n_src) % 6]
    counts[3] = 25                                                                    # the hub source is an overflow row
    X = np.zeros((n_src, 64), np.float32)
    for r in range(n_src):
        k = int(counts[r])
        cols = rng.permutation(64)[:k]
        if 2 <= k < 64 and r % 2:
            cols[:2] = [0, 63]
            cols[2:] = rng.permutation(np.arange(1, 63))[:k - 2]
        elif k == 1:
            cols[0] = (0, 63, 17)[r % 3]
        X[r, cols] = rng.choice([-8, -5, -3, -2, -1, 1, 2, 3, 4, 7, 8], k)
    assert np.array_equal((X != 0).sum(1), counts)
    sc = rng.choice([-3, -2, -1, 1, 2, 3], n_src).astype(np.float32)
    Xs = X * sc[:, None]
    x = T(X, DEV)
    assert be.rows_slots_supported(x, view_of(csr))
    slots, ovf = be.rows_slots_pack(x)
    ref_slots, over = _reference_slots(X)
    assert int(ovf) == over == int((counts > 24).sum()) and np.array_equal(N(slots).view(np.uint32), ref_slots)
    scaled, ovf2 = be.rows_slots_pack(x, row_scale=T(sc, DEV))
    ref_scaled, _ = _reference_slots(Xs)
    assert int(ovf2) == over and np.array_equal(N(scaled).view(np.uint32), ref_scaled)
    big = counts > 24
    empty = np.zeros(32, np.uint32)
    empty[0::4] = 0xFF404040
    assert bool((N(scaled).view(np.uint32)[big] == empty[None, :]).all())              # overflow rows: the flag, no values
    want, want_s = exact_pair(dst, n_dst, lambda c: X[:, c][src], 64), exact_pair(dst, n_dst, lambda c: Xs[:, c][src], 64)
    for name, v in gpu_views(csr, splits=(64, 256)):
        for red in ("sum", "mean"):
            out = torch.full((n_dst, 64), float("nan"), device=DEV)
            be.spmm_copy_u_strided(v, red, x, out, slots=slots)
            assert last_kernel() == "slots", name
            (assert_exact if red == "sum" else lambda g_, w_, m_: assert_mean(g_, w_, deg, m_))(N(out), want, "slots %s %s" % (red, name))
        out = torch.full((n_dst, 64), float("nan"), device=DEV)
        be.spmm_copy_u_strided(v, "sum", x, out, slots=scaled, src_scale=T(sc, DEV))
        assert last_kernel() == "slots"
        assert_exact(N(out), want_s, "slots with a row factor " + name)
        base, ds = ints(rng, (n_dst, 128), 8), ints(rng, n_dst, 3)
        wide = T(base, DEV)
        be.spmm_copy_u_strided(v, "sum", x, wide[:, 64:], accumulate=True, dst_scale=T(ds, DEV), slots=slots)
        assert_exact(N(wide[:, 64:]), base[:, 64:].astype(np.int64) + ds.astype(np.int64)[:, None] * want, "slots accumulate " + name)
        assert torch.equal(wide[:, :64], T(base, DEV)[:, :64])


@pytest.mark.gpu
def test_edge_tail_kernel_on_the_ladder():
    for bip in (False, True):
        G = ladder(bip)
        src, dst, n_src, n_dst = G
        deg = degrees(G)
        csr = make_csr(G, torch.int32, DEV)
        be = sparse.backend_for(csr.indptr)
        rng = np.random.default_rng(12)
        Xw = ints(rng, (n_src, 200), 8)
        X = np.ascontiguousarray(Xw[:, :100])
        x = T(Xw, DEV)[:, :100]
        want = exact_pair(dst, n_dst, lambda c: X[:, c][src], 100)
        for name, v in gpu_views(csr, splits=(64, 256)):
            operands = be.edge_tail_of(v, x)
            assert operands is not None
            a, tail = operands
            assert torch.equal(a, x[:, :96]) and torch.equal(tail, x[:, 96:][v.indices.long()])
            for red in ("sum", "mean"):
                out = torch.full((n_dst, 100), float("nan"), device=DEV)
                be.spmm_copy_u_edge_tail(v, red, a, tail, out)
                assert last_kernel() == "edge tail"
                (assert_exact if red == "sum" else lambda g_, w_, m_: assert_mean(g_, w_, deg, m_))(N(out), want, "edge tail %s %s" % (red, name))
            base, ds = ints(rng, (n_dst, 200), 8), ints(rng, n_dst, 3)
            buf = T(base, DEV)
            be.spmm_copy_u_edge_tail(v, "sum", a, tail, buf[:, 100:], accumulate=True, dst_scale=T(ds, DEV))
            assert_exact(N(buf[:, 100:]), base[:, 100:].astype(np.int64) + ds.astype(np.int64)[:, None] * want, "edge tail accumulate " + name)
            assert torch.equal(buf[:, :100], T(base, DEV)[:, :100])


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3, 8, 16])
def test_rel_kernels_on_the_ladder(R):
    """mgx_spmm_rel / mgx_spmm_rel_grad with integer weights per (position, relation), permuted from edge-id order by mgx_gather_rows: a
    wrong permutation is an exact mismatch.  idtype alternates with D."""
    G = ladder(True)
    src, dst, n_src, n_dst = G
    nnz = src.shape[0]
    deg = degrees(G)
    rng = np.random.default_rng(R)
    W = ints(rng, (nnz, R), 4)
    for D, idtype in ((1, torch.int32), (4, torch.int64), (32, torch.int32), (64, torch.int64))[:4 if R < 16 else 2] + (((64, torch.int32),) if R == 16 else ()):
        csr = make_csr(G, idtype, DEV)
        rev = sparse.csr_transpose(csr)                       # rows = sources
        be = sparse.backend_for(csr.indptr)
        X, dZ = ints(rng, (n_src, D), 8), ints(rng, (n_dst, R, D), 8)
        want = np.stack([exact_pair(dst, n_dst, lambda c, r=r: X[:, c][src] * W[:, r:r + 1], D) for r in range(R)], 1)
        dZ2 = dZ.reshape(n_dst, R * D)
        Wrep = lambda c: W[:, np.arange(c.start, c.stop) // D]
        per_r = exact_pair(src, n_src, lambda c: dZ2[:, c][dst] * Wrep(c), R * D)     # also bounds the sum over r: |a + b| <= |a| + |b|
        assert int(reduce_rows(src, n_src, lambda c: dZ2[:, c][dst] * Wrep(c), R * D, absolute=True).reshape(n_src, R, D).sum(1).max()) < xl.LIMIT
        want_dx = per_r.reshape(n_src, R, D).sum(1)
        x, w = T(X, DEV), T(W, DEV)
        for kind, split in (("none", 0), ("natural", 64), ("shuffled", 256)):
            v, vt = view_of(csr, kind, split), view_of(rev, kind, split)
            assert (v.plan() is None) == (kind == "none")
            w_pos, w_pos_t = be.gather_rows(w, v.eids), be.gather_rows(w, vt.eids)
            what = "rel R=%d D=%d %s/%d" % (R, D, kind, split)
            assert_exact(N(be.spmm_rel(v, "sum", w_pos, x)), want, what)
            assert last_kernel() == "rel"
            assert_mean(N(be.spmm_rel(v, "mean", w_pos, x)), want, deg, what + " mean")
            assert_exact(N(be.spmm_rel_grad(vt, w_pos_t, T(dZ, DEV))), want_dx, what + " grad")
            assert last_kernel() == "rel_grad"


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_autograd_on_the_ladder(idtype, monkeypatch):
    monkeypatch.setenv("MGX_SCHEDULE", "natural")
    monkeypatch.setattr(mgx_config, "HUB_SPLIT", 64)
    G = ladder(True)
    g = graph_of(G, idtype, DEV)
    autograd_cases(G, g, DEV)
    if idtype == torch.int32:
        assert g._index.csc().plan().num_hubs >= 1 and g._index.csr().plan().num_hubs >= 1


# ============================================================================= GPU: edge softmax and GAT attention
@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 8, 64])
def test_edge_softmax_and_gat_attention_exact_forms(H):
    G = ladder(False)
    be = sparse.backend_for(torch.zeros(1, device=DEV))
    for idtype in (torch.int32, torch.int64):
        csr = make_csr(G, idtype, DEV)
        for kind, split in (("none", 256), ("natural", 64), ("natural", 256), ("shuffled", 256)):
            if idtype == torch.int64 and kind == "shuffled":
                continue
            softmax_uniform_case(be, view_of(csr, kind, split), G, H, DEV)
            softmax_one_hot_case(be, G, H, DEV, idtype, lambda c, k=kind, s=split: view_of(c, k, s), split,
                                 rounds=range(16 if idtype == torch.int32 else 4))


def _close_rows(out, ref, row_scale):
    from test_gpu_fuzz import close_rows
    return close_rows(out, ref, row_scale)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 8])
def test_softmax_and_attention_backward_against_fp64(H, monkeypatch):
    """No exact form: fp64 references, the row-scaled 1e-4 bound of test_gpu_fuzz.close_rows (1e-4 x the sum of |terms| of that row)."""
    G = ladder(False)
    src, dst, n, _ = G
    nnz = src.shape[0]
    rng = np.random.default_rng(20 + H)
    for split, mode in ((64, "natural"), (256, "natural"), (256, "none")):
        monkeypatch.setenv("MGX_SCHEDULE", mode)
        monkeypatch.setattr(mgx_config, "HUB_SPLIT", split)
        g = graph_of(G, torch.int32, DEV)
        z = (rng.standard_normal((nnz, H, 1)) * 3).astype(np.float32)
        da = rng.standard_normal((nnz, H, 1)).astype(np.float32)

        def reference(z64, da64):
            m = np.full((n, H), -np.inf)
            np.maximum.at(m, dst, z64)
            e = np.exp(z64 - m[dst])
            s = np.zeros((n, H))
            np.add.at(s, dst, e)
            a = e / s[dst]
            dot, mag = np.zeros((n, H)), np.zeros((n, H))
            np.add.at(dot, dst, a * da64)
            np.add.at(mag, dst, np.abs(a * da64))
            return a, a * (da64 - dot[dst]), a * (np.abs(da64) + mag[dst])

        a64, dz64, bound = reference(z.reshape(nnz, H).astype(np.float64), da.reshape(nnz, H).astype(np.float64))
        zt = T(z, DEV).requires_grad_(True)
        a = ops.edge_softmax(g, zt)
        assert _close_rows(N(a).reshape(nnz, H), a64, np.ones_like(a64))
        (a * T(da, DEV)).sum().backward()
        assert _close_rows(N(zt.grad).reshape(nnz, H), dz64, bound), ("edge_softmax backward", H, split, mode)
        el = rng.standard_normal((n, H, 1)).astype(np.float32)
        er = rng.standard_normal((n, H, 1)).astype(np.float32)
        t = (el[src] + er[dst]).astype(np.float32).reshape(nnz, H).astype(np.float64)   # the fp32 sum the kernel forms, then fp64
        slope = 0.2
        a64, dz64, bound = reference(np.where(t > 0, t, slope * t), da.reshape(nnz, H).astype(np.float64))
        dzz = dz64 * np.where(t > 0, 1.0, slope)
        elt, ert = T(el, DEV).requires_grad_(True), T(er, DEV).requires_grad_(True)
        af = ops.gat_attention(g, elt, ert, slope)
        assert _close_rows(N(af).reshape(nnz, H), a64, np.ones_like(a64))
        (af * T(da, DEV).view(af.shape)).sum().backward()
        want_l, want_r, mag_l, mag_r = (np.zeros((n, H)) for _ in range(4))
        np.add.at(want_l, src, dzz)
        np.add.at(want_r, dst, dzz)
        np.add.at(mag_l, src, bound)
        np.add.at(mag_r, dst, bound)
        assert _close_rows(N(elt.grad).reshape(n, H), want_l, mag_l), ("gat_attention d el", H, split, mode)
        assert _close_rows(N(ert.grad).reshape(n, H), want_r, mag_r), ("gat_attention d er", H, split, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("H,F", [(1, 16), (4, 8), (8, 4), (1, 41), (2, 64)])
def test_fused_gat_layer_forward_and_backward_against_fp64(H, F, monkeypatch):
    """ops.gat_fused (csrc/gatfused.hip, attn_drop = 0) on the ladder graph: no plan, plans with hub rows at HUB_SPLIT 64 and 256, and
    the tile walks where the head width has one.  Signed inputs, fp64 references, every element within 1e-4 x the sum of |terms|
    reduced into it (test_gpu_fuzz.close_rows)."""
    G = ladder(False)
    src, dst, n, _ = G
    nnz = src.shape[0]
    rng = np.random.default_rng(40 + H + F)
    feat = rng.standard_normal((n, H, F)).astype(np.float32)
    el, er = rng.standard_normal((n, H, 1)).astype(np.float32), rng.standard_normal((n, H, 1)).astype(np.float32)
    up = rng.standard_normal((n, H, F)).astype(np.float32)
    slope = 0.2
    f64, u64 = feat.astype(np.float64), up.astype(np.float64)
    t = (el[src] + er[dst]).astype(np.float32).reshape(nnz, H).astype(np.float64)      # the fp32 sum the kernels form, then fp64
    z = np.where(t > 0, t, slope * t)
    m = np.full((n, H), -np.inf)
    np.maximum.at(m, dst, z)
    e = np.exp(z - m[dst])
    ssum = np.zeros((n, H))
    np.add.at(ssum, dst, e)
    a = e / ssum[dst]
    out64, out_mag = np.zeros((n, H, F)), np.zeros((n, H, F))
    np.add.at(out64, dst, a[:, :, None] * f64[src])
    np.add.at(out_mag, dst, a[:, :, None] * np.abs(f64[src]))
    dfeat64, dfeat_mag = np.zeros((n, H, F)), np.zeros((n, H, F))
    np.add.at(dfeat64, src, a[:, :, None] * u64[dst])
    np.add.at(dfeat_mag, src, a[:, :, None] * np.abs(u64[dst]))
    da = (f64[src] * u64[dst]).sum(-1)
    da_mag = (np.abs(f64[src]) * np.abs(u64[dst])).sum(-1)
    dot, dot_mag = np.zeros((n, H)), np.zeros((n, H))
    np.add.at(dot, dst, a * da)
    np.add.at(dot_mag, dst, a * da_mag)
    dt = a * (da - dot[dst]) * np.where(t > 0, 1.0, slope)
    dt_mag = a * (da_mag + dot_mag[dst])
    del64, der64, del_mag, der_mag = (np.zeros((n, H)) for _ in range(4))
    np.add.at(del64, src, dt)
    np.add.at(der64, dst, dt)
    np.add.at(del_mag, src, dt_mag)
    np.add.at(der_mag, dst, dt_mag)
    for mode, split, tile in (("none", 256, "0"), ("natural", 64, "0"), ("natural", 256, "0"), ("natural", 256, "1")):
        if tile == "1" and not (F % 4 == 0 and 4 <= F <= 16):
            continue
        monkeypatch.setenv("MGX_SCHEDULE", mode)
        monkeypatch.setattr(mgx_config, "HUB_SPLIT", split)
        monkeypatch.setenv("MGX_TILE", tile)
        monkeypatch.setenv("MGX_GAT_TILE", tile)
        g = graph_of(G, torch.int32, DEV)
        ins = [T(v, DEV).requires_grad_(True) for v in (feat, el, er)]
        assert ops.gat_fused_supported(g, ins[0])
        out = ops.gat_fused(g, ins[0], ins[1], ins[2], slope, 0.0, True)
        what = (H, F, mode, split, tile)
        plan = g._index.csc().plan()
        assert (plan is None) == (mode == "none") and (plan is None or plan.num_hubs >= 1)
        assert (g._index.csc().gat_tile_plan(F) is not None) == (tile == "1")
        assert _close_rows(N(out), out64, out_mag), ("gat_fused forward",) + what
        out.backward(T(up, DEV))
        assert _close_rows(N(ins[0].grad), dfeat64, dfeat_mag), ("gat_fused d feat",) + what
        assert _close_rows(N(ins[1].grad).reshape(n, H), del64, del_mag), ("gat_fused d el",) + what
        assert _close_rows(N(ins[2].grad).reshape(n, H), der64, der_mag), ("gat_fused d er",) + what


# ============================================================================= GPU: the other fixed-order reductions
@pytest.mark.gpu
def test_segment_reduce_with_ladder_segments():
    lens = xl.ladder_lengths(seed=3)
    total = int(lens.sum())
    seg = np.repeat(np.arange(lens.shape[0]), lens)
    rng = np.random.default_rng(13)
    for D in (1, 7, 64, 100):
        X = ints(rng, (total, D), 8)
        want = exact_pair(seg, lens.shape[0], lambda c: X[:, c], D)
        x = T(X, DEV)
        seglen = torch.from_numpy(lens).to(DEV)
        assert_exact(N(ops.segment_reduce(seglen, x, "sum")), want, "segment sum D=%d" % D)
        assert_mean(N(ops.segment_reduce(seglen, x, "mean")), want, lens, "segment mean D=%d" % D)
        for red, fn, ident in (("max", np.maximum, -99), ("min", np.minimum, 99)):
            ref = np.full((lens.shape[0], D), ident, np.int64)
            fn.at(ref, seg, X.astype(np.int64))
            ref[lens == 0] = 0
            assert_exact(N(ops.segment_reduce(seglen, x, red)), ref, "segment %s D=%d" % (red, D))


@pytest.mark.gpu
@pytest.mark.parametrize("n,C", [(1, 1), (63, 7), (4097, 64), (70001, 100), (300000, 16), (123457, 256)])
def test_column_sum_exact(n, C):
    X = ints(np.random.default_rng(n + C), (n, C), 8)
    assert int(np.abs(X).astype(np.int64).sum(0).max()) < xl.LIMIT
    x = T(X, DEV)
    assert_exact(N(sparse.backend_for(x).column_sum(x)), X.astype(np.int64).sum(0), "column_sum")


XTY_SHAPES = [(0, 3, 5), (1, 1, 1), (5, 64, 128), (1000, 47, 64), (70001, 64, 100), (300000, 16, 7), (123457, 33, 113), (65536, 64, 64),
              (70000, 256, 128), (66000, 200, 300), (3000, 65, 129), (80000, 128, 602), (70000, 256, 1024), (50, 256, 1000),
              (169343, 256, 512), (0, 200, 300)]                                     # test_gpu_parity.test_xty_matches_fp64
XTY_COLSUM_SHAPES = [(70001, 64, 128), (65537, 64, 200), (100000, 47, 128), (70000, 64, 64), (66000, 16, 100), (5000, 64, 128),
                     (70000, 64, 72), (70000, 128, 128), (0, 64, 128)]              # test_xty_with_column_sums_matches_fp64


def _xty_operands(n, M, K):
    """Values in [-3, 3]: 300 000 x 9 < 2^24.  The reference product is formed in fp64, where these integers and their sums are exact."""
    rng = np.random.default_rng(n + M + K)
    A, B = ints(rng, (n, M), 3), ints(rng, (n, K), 3)
    assert float((np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64)).max(initial=0.0)) < xl.LIMIT
    return A, B, np.rint(A.astype(np.float64).T @ B.astype(np.float64)).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("n,M,K", XTY_SHAPES)
def test_xty_is_plain_fp32_on_integers(n, M, K):
    """mgx_xty at test_gpu_parity's shapes, the K = 1024 limit included.  A mismatch would mean the MFMA path is not plain fp32."""
    A, B, want = _xty_operands(n, M, K)
    a, b = T(A, DEV), T(B, DEV)
    assert_exact(N(sparse.backend_for(a).xty(a, b)), want, "xty")


@pytest.mark.gpu
@pytest.mark.parametrize("n,M,K", XTY_COLSUM_SHAPES + [(300000, 16, 7), (70000, 256, 1024)])
def test_xty_colsum_is_plain_fp32_on_integers(n, M, K):
    """backend.xty(colsum=True): mgx_xty_colsum where it applies, else mgx_xty + mgx_column_sum; also from a row-strided first operand."""
    A, B, want = _xty_operands(n, M, K)
    a, b = T(A, DEV), T(B, DEV)
    be = sparse.backend_for(a)
    got, sums = be.xty(a, b, colsum=True)
    assert_exact(N(got), want, "xty with column sums")
    assert_exact(N(sums), A.astype(np.int64).sum(0), "column sums of xty")
    wide = torch.cat([a, torch.full((n, 8), 5.0, device=DEV)], 1)
    got, sums = be.xty(wide[:, :M], b, colsum=True)
    assert_exact(N(got), want, "xty with column sums, strided")
    assert_exact(N(sums), A.astype(np.int64).sum(0), "column sums of xty, strided")


_xty_small = {}


def _xty_small_operands(n):
    """One [n, 64] x [n, 128] pair per n (values in [-3, 3], 4117 x 9 < 2^24) with its exact product, made once and never written:
    the cases below take columns of it.  n = 37: a ragged last step, and 253 of the 256 waves have no row.  n = 4117: xty_waves
    gives 256 waves, one sweep covers 4096 rows, so wave 0 makes a full second trip and wave 1 a ragged one."""
    if n not in _xty_small:
        A, B, want = _xty_operands(n, 64, 128)
        _xty_small[n] = (A, want, T(A, DEV), T(B, DEV))
    return _xty_small[n]


@pytest.mark.gpu
@pytest.mark.parametrize("kt", range(1, 9))
@pytest.mark.parametrize("mt", range(1, 5))
@pytest.mark.parametrize("n", [37, 4117])
def test_xty_every_dword_instantiation(n, mt, kt):
    """The dword-load kernel <mt, kt> with ragged last tiles; a row stride of K = 16 kt - 1 floats can never take the 16-byte form."""
    M, K = 16 * mt - 3, 16 * kt - 1
    _, want, a, b = _xty_small_operands(n)
    a, b = a[:, :M].contiguous(), b[:, :K].contiguous()
    assert_exact(N(sparse.backend_for(a).xty(a, b)), want[:M, :K], "xty, dword form <%d, %d>" % (mt, kt))


@pytest.mark.gpu
def test_xty_dword_form_through_a_misaligned_view():
    """K % 4 == 0 and a row stride of 128 floats, but the view starts one float in: 4-byte aligned only, so the dword form <4, 4>;
    with colsum=True mgx_xty_colsum has no kernel for it and the sums come from mgx_column_sum."""
    A, want, a, wide = _xty_small_operands(4117)
    b = wide[:, 1:65]
    assert b.data_ptr() % 16 == 4 and b.stride(0) % 4 == 0
    be = sparse.backend_for(a)
    assert_exact(N(be.xty(a, b)), want[:, 1:65], "xty, misaligned b")
    got, sums = be.xty(a, b, colsum=True)
    assert_exact(N(got), want[:, 1:65], "xty with column sums, misaligned b")
    assert_exact(N(sums), A.astype(np.int64).sum(0), "column sums of xty, misaligned b")


@pytest.mark.gpu
@pytest.mark.parametrize("n,M,K", [(37, 65, 129),        # four tiles, ragged in both directions, almost every wave without a row
                                   (4117, 200, 300)])   # twelve tiles, 64 waves per tile: five trips, the last one ragged
def test_xty_grid_of_tiles_at_small_n(n, M, K):
    A, B, want = _xty_operands(n, M, K)
    a, b = T(A, DEV), T(B, DEV)
    assert_exact(N(sparse.backend_for(a).xty(a, b)), want, "xty, grid of tiles")


@pytest.mark.gpu
def test_xty_two_tiles_one_launch_each_with_column_sums():
    """64 x 200: a 64 x 128 and a 64 x 72 tile, one launch each; the column sums come with the first."""
    A, B, want = _xty_operands(4117, 64, 200)
    a, b = T(A, DEV), T(B, DEV)
    got, sums = sparse.backend_for(a).xty(a, b, colsum=True)
    assert_exact(N(got), want, "xty, two tiles")
    assert_exact(N(sums), A.astype(np.int64).sum(0), "column sums of xty, two tiles")


@pytest.mark.gpu
@pytest.mark.parametrize("K,M,bt,lda_pad,n", [(200, 64, True, 0, 70001), (128, 64, True, 0, 65600), (128, 47, True, 0, 66000),
                                              (64, 128, False, 0, 70000), (47, 128, False, 0, 65599), (64, 128, False, 8, 5000),
                                              (41, 128, False, 0, 333), (32, 64, True, 0, 17), (256, 64, True, 0, 4097)])
def test_rows_gemm_is_plain_fp32_on_integers(K, M, bt, lda_pad, n):
    rng = np.random.default_rng(K + M + n)
    A, B = ints(rng, (n, K + lda_pad), 3), ints(rng, (M, K) if bt else (K, M), 3)
    bias, rs = ints(rng, M, 8), ints(rng, n, 3)
    Bm = (B.T if bt else B).astype(np.float64)
    prod = np.rint(A[:, :K].astype(np.float64) @ Bm).astype(np.int64)
    assert float((np.abs(A[:, :K]).astype(np.float64) @ np.abs(Bm)).max()) * 3 + 8 < xl.LIMIT
    be = sparse.backend_for(torch.zeros(1, device=DEV))
    a, b = T(A, DEV)[:, :K], T(B, DEV)
    if not be.rows_gemm_supported(K, M, a.stride(0)):
        assert be.rows_gemm(a, b, b_transposed=bt) is None
        return
    assert_exact(N(be.rows_gemm(a, b, b_transposed=bt)), prod, "rows_gemm")
    full = (prod + bias.astype(np.int64)[None, :]) * rs.astype(np.int64)[:, None]
    assert_exact(N(be.rows_gemm(a, b, b_transposed=bt, bias=T(bias, DEV), row_scale=T(rs, DEV), scale_from=0)), full, "rows_gemm + bias, row scale")


@pytest.mark.gpu
def test_scatter_add_rows_and_unpack_add_csr_exact():
    rng = np.random.default_rng(14)
    be = sparse.backend_for(torch.zeros(1, device=DEV))
    for D in (1, 7, 64, 100):
        for idt in (np.int32, np.int64):
            base, rows = ints(rng, (5000, D), 8), ints(rng, (3000, D), 8)
            idx = rng.permutation(5000)[:3000].astype(idt)
            x = T(base, DEV)
            be.scatter_add_rows(x, T(idx, DEV), T(rows, DEV))
            want = base.astype(np.int64)
            want[idx] += rows.astype(np.int64)
            assert_exact(N(x), want, "scatter_add_rows D=%d" % D)
    lens = xl.ladder_lengths(seed=4, repeats=2, thresholds=[64], longest=0)        # owners with ladder-many packed rows each
    n_own, n_sent = lens.shape[0], int(lens.sum())
    owner = np.repeat(np.arange(n_own), lens)
    pos = rng.permutation(n_sent)
    for D in (16, 64, 100):
        X = ints(rng, (n_sent, D), 8) * (rng.random((n_sent, D)) < 0.25)
        xt = T(X.astype(np.float32), DEV)
        masks, counts = be.rows_pack_count(xt, None)
        off = torch.zeros(n_sent + 1, dtype=torch.int64, device=DEV)
        torch.cumsum(counts, 0, dtype=torch.int64, out=off[1:])
        vals = be.rows_pack_values(xt, None, masks, off, int(off[-1]))
        csr = sparse.coo_to_csr(n_own, n_sent, torch.from_numpy(owner.astype(np.int32)).to(DEV), torch.from_numpy(pos.astype(np.int32)).to(DEV))
        base = ints(rng, (n_own, D + 4), 8)
        out = T(base, DEV)
        be.rows_unpack_add_csr(csr, masks, off, vals, out[:, :D])
        want = base[:, :D].astype(np.int64) + exact_pair(owner, n_own, lambda c: X[:, c][pos], D)
        assert_exact(N(out[:, :D]), want, "rows_unpack_add_csr D=%d" % D)
        assert torch.equal(out[:, D:], T(base, DEV)[:, D:])


@pytest.mark.gpu
@pytest.mark.parametrize("H,F", [(1, 4), (1, 64), (8, 8), (3, 4), (1, 41), (2, 128), (1, 7)])
def test_gsddmm_dot_exact_on_both_walks(H, F):
    G = ladder(True)
    src, dst, n_src, n_dst = G
    rng = np.random.default_rng(H * 100 + F)
    U, V = ints(rng, (n_src, H, F), 8), ints(rng, (n_dst, H, F), 8)
    assert H * F * 64 < xl.LIMIT
    want = (U[src].astype(np.int64) * V[dst].astype(np.int64)).sum(-1, keepdims=True)
    g = graph_of(G, torch.int32, DEV)
    for gi in (g, g.formats(["csr", "csc"])):
        assert_exact(N(ops.gsddmm(gi, "dot", T(U, DEV), T(V, DEV), "u", "v")), want, "dot H=%d F=%d" % (H, F))
        assert_exact(N(ops.gsddmm(gi, "dot", T(V, DEV), T(U, DEV), "v", "u")), want, "dot v, u H=%d F=%d" % (H, F))
