"""Value edges: ties, signed zeros, infinities, NaN, masked (-inf) logits and wide-range logits -- where test_exact_structure.py and
the fp64 parity tests use tame values.  References are plain numpy fp64 over the COO list (value_edges.py), formed from the fp32
numbers the kernels see.

1. max / min reducers.  The contract of mgx_spmm_csr (include/mi355x_graph.h), shared by spmm_generic_kernel, the OpenMP backend and
   oracle.c: a strict compare from the identity in CSR storage order, so the FIRST extremum wins (for a CSR built from COO: the
   smallest edge id), +0.0 and -0.0 tie, a NaN never wins, and a non-empty row whose terms never beat the identity keeps it with
   args -1.  Values are compared bit for bit, arg_e / arg_u exactly, the backward routes every gradient to the reference arg.
2. The softmax family at wide logit range on a private-source graph (every edge its own source: the test decides what sits at which
   CSR position): shifts of +-90 and +-3e4, ramps of 25 per rank, one dominant edge at +200 on every step / chunk edge, underflowing
   edges, a row of 88s.  The bound is test_gpu_fuzz.close_rows' 1e-4 x the sum of |terms|, unchanged.
3. Masked logits: about 30 % of every row at -inf, at the head, the tail, a lane group's whole share, scattered.  Masked edges get
   exactly 0 and exactly-0 gradients, whatever their position.
4. One NaN source and one +inf source reach exactly the destinations the graph sends them to, in every copy_u sum / mean family.

CPU (no marker): the OpenMP backend and the oracle.  GPU (-m gpu): the HIP kernels."""
import numpy as np
import pytest
import torch

from mi355x_graph import config as mgx_config, ops, schedule, sparse, tileplan

import exact_ladder as xl
import value_edges as ve
from exact_ladder import exact_pair, ints
from test_exact_structure import DEV, GROUPS, N, T, cpu_on, degrees, gpu_views, graph_of, ladder, last_kernel, make_csr, memo, view_of  # noqa: F401
from test_gpu_fuzz import close_rows

K_TIE = 4


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ============================================================================= 1. max / min
def max_min_forms(G):
    """name -> (op, U | None, E | None, term [nnz, K] fp32): the plain forms and the offset-table form (N, 1, F) + (E, H, 1).  The
    edge-valued forms carry the designed ties and special values of value_edges; the source-valued ones small integer ranges."""
    def make():
        src, dst, n_src, n_dst = G
        nnz = src.shape[0]
        E = np.concatenate([ve.edge_tie_values(dst, n_dst, K_TIE, 1), ve.edge_special_values(dst, n_dst, 2)], 1)
        X = ve.node_tie_values(n_src, K_TIE, 3)
        forms = {"copy_rhs": ("copy_rhs", None, E, E), "copy_lhs": ("copy_lhs", X, None, X[src])}
        Ea = E[:, :X.shape[1]].copy()
        Ea[:, K_TIE + 1:] = ints(np.random.default_rng(4), (nnz, X.shape[1] - K_TIE - 1), 2)
        with np.errstate(invalid="ignore"):
            forms["add"] = ("add", X, Ea, (X[src] + Ea).astype(np.float32))          # +inf + -inf: NaN terms too
            Em = ints(np.random.default_rng(5), Ea.shape, 2)
            Em[:, K_TIE + 1] = np.where(np.arange(nnz) % 3 == 0, 0.0, Em[:, K_TIE + 1])   # 0 x inf among the terms
            forms["mul"] = ("mul", X, Em, (X[src] * Em).astype(np.float32))
            H, F = 3, 2
            Ub = np.random.default_rng(6).integers(0, 2, (n_src, 1, F)).astype(np.float32)
            Eb = np.stack([ve.edge_tie_values(dst, n_dst, 2, 7)[:, 0], ve.edge_tie_values(dst, n_dst, 2, 8)[:, 1],
                           ve.edge_special_values(dst, n_dst, 9)[:, 2]], 1).reshape(nnz, H, 1)
            forms["add table"] = ("add", Ub, Eb, (Ub[src] + Eb).astype(np.float32).reshape(nnz, H * F))
        refs = {}
        for name, (op, U, Ev, term) in forms.items():
            for red in ("max", "min"):
                val, arg, tie = ve.first_extremum(dst, n_dst, term, red)
                refs[name, red] = (val, arg)
                live = np.repeat((degrees(G) > 0)[:, None], term.shape[1], 1)
                # from the reference alone: ties are the normal case here, and the special rows exist
                assert int(tie[live].sum()) * 2 >= int(live.sum()), (name, red, int(tie[live].sum()), int(live.sum()))
                assert bool(((arg == -1) & live).any()) and bool(np.isinf(val[live]).any()), (name, red)
        val, arg, tie = ve.first_extremum(dst, n_dst, E, "max")
        lens = degrees(G)
        assert bool(tie[(np.arange(n_dst) % 5 == 2) & (lens > 2), 0].all()) and bool(tie[(np.arange(n_dst) % 5 == 3) & (lens > 64), 0].all())
        relu = E[:, :K_TIE][dst % 5 == 1]
        assert float((relu == 0).mean()) >= 0.7 and float(relu.min()) == 0.0
        return forms, refs
    return memo(G, "max/min forms", make)


def check_selection(what, out, arg_u, arg_e, ref, src, op):
    val, arg = ref
    assert np.array_equal(bits(out).reshape(val.shape), bits(val)), (what, "values", int((bits(out).reshape(val.shape) != bits(val)).sum()))
    if op != "copy_lhs":
        assert np.array_equal(np.asarray(arg_e, np.int64).reshape(arg.shape), arg), (what, "arg_e")
    if op != "copy_rhs":
        assert np.array_equal(np.asarray(arg_u, np.int64).reshape(arg.shape), np.where(arg >= 0, src[np.maximum(arg, 0)], -1)), (what, "arg_u")


def max_min_value_cases(views, G, dev, kernel=None):
    forms, refs = max_min_forms(G)
    src = G[0]
    for vname, view in views:
        assert np.array_equal(N(view.eids), np.argsort(G[1], kind="stable"))      # storage order inside a row is edge-id order
        for name, (op, U, E, _) in forms.items():
            for red in ("max", "min"):
                out, au, ae = sparse.gspmm_raw(view, op, red, None if U is None else T(U, dev), None if E is None else T(E, dev), want_arg=True)
                if kernel is not None:
                    assert last_kernel() == kernel, (name, red, vname, last_kernel())
                check_selection((name, red, vname), N(out), None if au is None else N(au), None if ae is None else N(ae), refs[name, red], src, op)


def max_min_backward_cases(G, g, dev, kernel=None):
    """ops.gspmm(..., max | min).backward with an integer upstream gradient: every (row, column) gradient lands on the reference
    arg's source / edge alone, rows with arg -1 contribute nothing."""
    forms, refs = max_min_forms(G)
    src, dst, n_src, n_dst = G
    nnz = src.shape[0]
    rng = np.random.default_rng(12)
    for name in ("copy_lhs", "copy_rhs", "add", "mul"):
        op, U, E, _ = forms[name]
        if name == "mul":                                                   # finite operands: the factors enter the gradient
            U, E = U[:, :K_TIE + 1], E[:, :K_TIE + 1]
        K = (U if U is not None else E).shape[1]
        dZ = ints(rng, (n_dst, K), 8)
        for red in ("max", "min"):
            if name == "mul":
                _, arg, _ = ve.first_extremum(dst, n_dst, (U[src] * E).astype(np.float32), red)
            else:
                arg = refs[name, red][1]
            won = arg >= 0
            r, c = np.nonzero(won)
            x = None if U is None else T(U, dev).requires_grad_(True)
            e = None if E is None else T(E, dev).requires_grad_(True)
            ops.gspmm(g, op, red, x, e).backward(T(dZ, dev))
            if kernel is not None:
                assert last_kernel() == kernel, (name, red, last_kernel())
            gx = dZ[r, c].astype(np.int64) * (E[arg[r, c], c].astype(np.int64) if name == "mul" else 1)
            ge = dZ[r, c].astype(np.int64) * (U[src[arg[r, c]], c].astype(np.int64) if name == "mul" else 1)
            if x is not None:
                want = np.zeros((n_src, K), np.int64)
                np.add.at(want, (src[arg[r, c]], c), gx)
                xl.assert_exact(N(x.grad), want, "%s %s X.grad" % (name, red))
                if name != "mul":
                    assert float(x.grad.sum()) == float(dZ[won].astype(np.int64).sum())
            if e is not None:
                want = np.zeros((nnz, K), np.int64)
                np.add.at(want, (arg[r, c], c), ge)
                xl.assert_exact(N(e.grad), want, "%s %s E.grad" % (name, red))
                if name != "mul":
                    assert float(e.grad.sum()) == float(dZ[won].astype(np.int64).sum())


def segment_value_cases(dev):
    """segment_reduce max / min on the same tie, infinity and NaN columns: a segment is a row whose edges are its own positions."""
    lens = xl.ladder_lengths(seed=3, repeats=1, thresholds=[64], longest=1500)
    seg = np.repeat(np.arange(lens.shape[0]), lens)
    X = np.concatenate([ve.edge_tie_values(seg, lens.shape[0], K_TIE, 21), ve.edge_special_values(seg, lens.shape[0], 22)], 1)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    for red in ("max", "min"):
        val, arg, tie = ve.first_extremum(seg, lens.shape[0], X, red)
        assert int(tie[lens > 0].sum()) * 2 >= int((lens > 0).sum()) * X.shape[1]
        out, got_arg = sparse.segment_reduce_raw(offsets, T(X, dev), red, want_arg=True)
        assert np.array_equal(bits(N(out)), bits(val)), ("segment", red)
        assert np.array_equal(N(got_arg), arg), ("segment arg", red)
        assert np.array_equal(bits(N(ops.segment_reduce(torch.from_numpy(lens).to(dev), T(X, dev), red))), bits(val))


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bipartite", [False, True])
def test_cpu_max_min_ties_zeros_infinities_nan(cpu_on, idtype, bipartite):
    G = ladder(bipartite)
    max_min_value_cases([("cpu", view_of(make_csr(G, idtype, "cpu")))], G, "cpu")


def test_oracle_max_min_ties_zeros_infinities_nan(oracle):
    for bip in (False, True):
        G = ladder(bip)
        src, dst, n_src, n_dst = G
        forms, refs = max_min_forms(G)
        ip, ix, ei = oracle.coo_to_csr(n_dst, dst, src)
        for name, (op, U, E, _) in forms.items():
            for red in ("max", "min"):
                out, au, ae = oracle.spmm(ip, ix, ei, op, red, U, E, want_arg=True)
                check_selection(("oracle", name, red), out, au if op != "copy_rhs" else None, ae, refs[name, red], src, "add" if op != "copy_rhs" else op)


def test_cpu_max_min_backward_and_segments(cpu_on):
    G = ladder(True)
    max_min_backward_cases(G, graph_of(G, torch.int32, "cpu"), "cpu")
    segment_value_cases("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bipartite", [False, True])
def test_generic_kernel_max_min_ties_zeros_infinities_nan(idtype, bipartite):
    G = ladder(bipartite)
    csr = make_csr(G, idtype, DEV)
    max_min_value_cases([("no plan", view_of(csr)), ("natural/256", view_of(csr, "natural", 256))], G, DEV, kernel="generic")


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_max_min_backward_routes_to_the_first_extremum(idtype, monkeypatch):
    monkeypatch.setenv("MGX_SCHEDULE", "natural")
    monkeypatch.setattr(mgx_config, "HUB_SPLIT", 64)
    G = ladder(True)
    g = graph_of(G, idtype, DEV)
    max_min_backward_cases(G, g, DEV, kernel="generic")            # the torch op drops the plan for max / min


@pytest.mark.gpu
def test_segment_reduce_max_min_ties_zeros_infinities_nan():
    segment_value_cases(DEV)


# ============================================================================= 2. / 3. the softmax family
PRIVATE = ve.private_graph()
LEGS = (("none", 256, "0"), ("natural", 64, "0"), ("natural", 256, "0"), ("natural", 256, "1"))
SLOPE = 0.25                        # exact in fp32: the logit of a negative sum is that sum's exact quarter


def private_lens():
    return degrees(PRIVATE)


def split_er(z, dst, n_dst, seed):
    """(el [n_src, H], er [n_dst, H]) with leaky_relu(fp32(el[u] + er[v])) = z on the private-source graph: er a small integer
    per row, el the pre-image of z minus er.  The two fp32 roundings can move a logit by an ulp, so every reference of the fused
    forms is formed from el and er again (gat_reference), never from z."""
    src = PRIVATE[0]
    er = np.random.default_rng(seed).integers(-2, 3, (n_dst, z.shape[1])).astype(np.float32)
    with np.errstate(invalid="ignore"):
        t = np.where(z > 0, z, z / np.float32(SLOPE)).astype(np.float32)
        el_e = (t - er[dst]).astype(np.float32)
    el = np.zeros_like(el_e)
    el[src] = el_e
    return el, er


def set_leg(monkeypatch, mode, split, tile):
    monkeypatch.setenv("MGX_SCHEDULE", mode)
    monkeypatch.setattr(mgx_config, "HUB_SPLIT", split)
    monkeypatch.setenv("MGX_TILE", tile)
    monkeypatch.setenv("MGX_GAT_TILE", tile)


def rounds_for(name):
    if name == "dominant":
        return range(max(len(ve.dominant_ranks(int(L))) for L in private_lens() if L))
    return range(1)


def check_unfused(g, G, z, H, dev, what, masked=None):
    """ops.edge_softmax and ops.gat_attention, forward and backward, against fp64 under the bounds of
    test_softmax_and_attention_backward_against_fp64.  Returns the attention."""
    src, dst, n_src, n_dst = G
    nnz = src.shape[0]
    rng = np.random.default_rng(31)
    da = rng.standard_normal((nnz, H)).astype(np.float32)
    a64, dz64, bound = ve.softmax_reference(dst, n_dst, z, da)
    ones = np.ones_like(a64)
    zt = T(z.reshape(nnz, H, 1), dev).requires_grad_(True)
    a = ops.edge_softmax(g, zt)
    got = N(a).reshape(nnz, H)
    assert np.isfinite(got).all(), what
    assert close_rows(got, a64, ones), ("edge_softmax",) + what
    (a * T(da.reshape(nnz, H, 1), dev)).sum().backward()
    dz = N(zt.grad).reshape(nnz, H)
    assert np.isfinite(dz).all() and close_rows(dz, dz64, bound), ("edge_softmax backward",) + what
    gone = ve.below_top(dst, n_dst, z) < -110
    if masked is not None:
        assert np.array_equal(gone, masked)
        assert not dz[masked].any(), ("edge_softmax: d z of a masked edge",) + what
    assert not got[gone].any(), ("edge_softmax: an edge 110 below the row's top must be exactly 0",) + what
    # the fused-logit form: the same z rebuilt from el[u] + er[v]
    el, er = split_er(z, dst, n_dst, 32)
    ref = ve.gat_reference(G, el, er, SLOPE, da=da)         # from its own fp32 sums el[u] + er[v]: z again, up to their rounding
    live = np.isfinite(z)
    assert np.array_equal(np.isfinite(ref["z"]), live) and float(np.max(np.abs(ref["z"][live] - z[live]) / np.maximum(np.abs(z[live]), 1), initial=0)) < 1e-6
    gone = ve.below_top(dst, n_dst, ref["z"]) < -110
    elt, ert = T(el.reshape(n_src, H, 1), dev).requires_grad_(True), T(er.reshape(n_dst, H, 1), dev).requires_grad_(True)
    af = ops.gat_attention(g, elt, ert, SLOPE)
    gotf = N(af).reshape(nnz, H)
    assert np.isfinite(gotf).all() and close_rows(gotf, ref["a"], ones), ("gat_attention",) + what
    assert not gotf[gone].any(), ("gat_attention: exactly 0",) + what
    (af * T(da.reshape(nnz, H, 1), dev).view(af.shape)).sum().backward()
    d_el, d_er = N(elt.grad).reshape(n_src, H), N(ert.grad).reshape(n_dst, H)
    assert np.isfinite(d_el).all() and np.isfinite(d_er).all(), what
    assert close_rows(d_el, ref["del"], ref["del_mag"]), ("gat_attention d el",) + what
    assert close_rows(d_er, ref["der"], ref["der_mag"]), ("gat_attention d er",) + what
    if masked is not None:
        assert not d_el[src][masked].any(), ("gat_attention: d el of a masked source",) + what
    return got, gotf


def unfused_wide_range(dev, H, legs, monkeypatch):
    G = PRIVATE
    src, dst, n_src, n_dst = G
    deg = private_lens()
    for mode, split in legs:
        monkeypatch.setenv("MGX_SCHEDULE", mode)
        monkeypatch.setattr(mgx_config, "HUB_SPLIT", split)
        g = graph_of(G, torch.int32, dev)
        if dev != "cpu":
            plan = g._index.csc().plan()
            assert (plan is None) == (mode == "none") and (plan is None or plan.num_hubs == int((deg > split).sum()) >= 1)
        for name in ve.PATTERNS:
            for rnd in list(rounds_for(name))[::(1 if H == 1 else 3)]:
                z = ve.logit_pattern(name, dst, n_dst, H, 50 + H, rnd)
                what = (name, rnd, H, mode, split)
                if name == "underflow":
                    top = np.full((n_dst, H), -np.inf)
                    np.maximum.at(top, dst, z.astype(np.float64))
                    assert int((z - top[dst] < -110).sum()) >= z.size // 4
                a, af = check_unfused(g, G, z, H, dev, what)
                if name == "ties at 88":
                    want = (np.float32(1) / deg[dst].astype(np.float32))[:, None].repeat(H, 1)
                    assert bool(xl.within_ulp(a, want, 1).all()) and bool(xl.within_ulp(af, want, 1).all()), what


def masked_coverage(masked, dst, n_dst):
    """From the mask alone: rank 0, the last rank, a whole first 64-edge step, a whole 64- and 256-edge hub chunk, a whole lane
    group's share (every fourth rank), and never a whole row."""
    nnz = dst.shape[0]
    rank = xl.rank_in_row(dst, np.arange(nnz))
    lens = np.bincount(dst, minlength=n_dst)
    seen = dict(first=0, last=0, step=0, chunk64=0, chunk256=0, share=0)
    for h in range(masked.shape[1]):
        m = masked[:, h]
        kept = np.bincount(dst, weights=(~m).astype(np.float64), minlength=n_dst)
        assert bool((kept[lens > 0] >= 1).all())
        frac = np.bincount(dst, weights=m.astype(np.float64), minlength=n_dst)[lens >= 2] / lens[lens >= 2]
        assert 0.2 <= float(frac.min()) and float(frac.max()) <= 0.5 and abs(float(frac[lens[lens >= 2] >= 15].mean()) - 0.3) < 0.03
        for v in np.nonzero(lens >= 2)[0]:
            mr = np.zeros(lens[v], bool)
            mr[rank[(dst == v) & m]] = True
            seen["first"] += bool(mr[0])
            seen["last"] += bool(mr[-1])
            seen["step"] += bool(lens[v] > 64 and mr[:64].all())
            seen["share"] += bool(lens[v] >= 8 and mr[0::4].all())
            for s in (64, 256):
                seen["chunk%d" % s] += bool(lens[v] > s and any(mr[b:b + s].all() for b in range(0, lens[v], s)))
    return seen


def unfused_masked(dev, H, legs, monkeypatch):
    """Section 3 on edge_softmax / gat_attention, then fully masked rows: NaN there (torch.softmax's answer), every other row the
    same bits as without them, and the same outcome under every schedule."""
    G = PRIVATE
    src, dst, n_src, n_dst = G
    deg = private_lens()
    seen_total = None
    full_rows = {}
    for mode, split in legs:
        monkeypatch.setenv("MGX_SCHEDULE", mode)
        monkeypatch.setattr(mgx_config, "HUB_SPLIT", split)
        g = graph_of(G, torch.int32, dev)
        for rnd in range(4 if H == 1 else 2):
            z, masked = ve.masked_logits(dst, n_dst, H, 60, rnd)
            seen = masked_coverage(masked, dst, n_dst)
            seen_total = seen if seen_total is None else {k: seen_total[k] + seen[k] for k in seen}
            check_unfused(g, G, z, H, dev, ("masked", rnd, H, mode, split), masked=masked)
        # fully masked rows: every second non-empty row, the 1000-edge row among them
        z, _ = ve.masked_logits(dst, n_dst, H, 60, 0)
        dead = (np.arange(n_dst) % 2 == 0) & (deg > 0)
        assert dead[np.argmax(deg)] and int(dead.sum()) >= 8 and int((~dead & (deg > 0)).sum()) >= 8
        base = N(ops.edge_softmax(g, T(z.reshape(-1, H, 1), dev))).reshape(-1, H)
        zd = z.copy()
        zd[dead[dst]] = -np.inf
        a = N(ops.edge_softmax(g, T(zd.reshape(-1, H, 1), dev))).reshape(-1, H)
        el, er = split_er(z, dst, n_dst, 32)
        attend = lambda l: N(ops.gat_attention(g, T(l.reshape(n_src, H, 1), dev), T(er.reshape(n_dst, H, 1), dev), SLOPE)).reshape(-1, H)
        eld = el.copy()
        eld[src[dead[dst]]] = -np.inf
        for got, alive in ((a, base), (attend(eld), attend(el))):
            assert np.isnan(got[dead[dst]]).all(), ("a fully masked row is NaN", H, mode, split)
            assert np.isfinite(alive).all() and np.array_equal(bits(got[~dead[dst]]), bits(alive[~dead[dst]])), ("other rows are unaffected", H, mode, split)
        full_rows[mode, split] = a
    first = next(iter(full_rows.values()))
    for key, a in full_rows.items():
        assert np.array_equal(np.isnan(a), np.isnan(first)) and close_rows(np.nan_to_num(a), np.nan_to_num(first), 2 * np.ones_like(a)), key
    assert min(seen_total.values()) >= 1, seen_total


UNFUSED_LEGS = (("none", 256), ("natural", 64), ("natural", 256))


@pytest.mark.parametrize("H", [1, 3, 8, 64])
def test_cpu_softmax_and_attention_wide_range(cpu_on, H, monkeypatch):
    unfused_wide_range("cpu", H, UNFUSED_LEGS[:1], monkeypatch)


@pytest.mark.parametrize("H", [1, 3, 8, 64])
def test_cpu_softmax_and_attention_masked_logits(cpu_on, H, monkeypatch):
    unfused_masked("cpu", H, UNFUSED_LEGS[:1], monkeypatch)


def test_oracle_softmax_wide_range_and_masked(oracle):
    src, dst, n_src, n_dst = PRIVATE
    ip, ix, ei = oracle.coo_to_csr(n_dst, dst, src)
    H = 3
    cases = [(name, ve.logit_pattern(name, dst, n_dst, H, 53, 1), None) for name in ve.PATTERNS]
    cases.append(("masked",) + ve.masked_logits(dst, n_dst, H, 60, 0))
    for name, z, masked in cases:
        a64 = ve.softmax_reference(dst, n_dst, z)
        a = oracle.edge_softmax_fwd(ip, ei, z)
        assert np.isfinite(a).all() and close_rows(a, a64, np.ones_like(a64)), name
        if masked is not None:
            assert not a[masked].any()
    zd = cases[-1][1].copy()
    zd[dst % 2 == 0] = -np.inf
    a = oracle.edge_softmax_fwd(ip, ei, zd)
    assert np.isnan(a[dst % 2 == 0]).all() and np.array_equal(bits(a[dst % 2 == 1]), bits(oracle.edge_softmax_fwd(ip, ei, cases[-1][1])[dst % 2 == 1]))


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 8, 64])
def test_softmax_and_attention_wide_range(H, monkeypatch):
    unfused_wide_range(DEV, H, UNFUSED_LEGS, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 8, 64])
def test_softmax_and_attention_masked_logits(H, monkeypatch):
    unfused_masked(DEV, H, UNFUSED_LEGS, monkeypatch)


# ----------------------------------------------------------------------------- the fused layer
def fused_operands(H, F, seed):
    src, dst, n_src, n_dst = PRIVATE
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_src, H, F)).astype(np.float32), rng.standard_normal((n_dst, H, F)).astype(np.float32)


def run_fused(g, G, el, er, feat, up, what, tile, masked=None, ref=None):
    """ops.gat_fused forward + backward against gat_reference under the fused-layer test's bounds, every number finite; then the
    composition it replaces (gat_attention, then gspmm(mul, sum)), which must agree with it within the sum of the two bounds."""
    src, dst, n_src, n_dst = G
    H, F = feat.shape[1:]
    ref = ve.gat_reference(G, el, er, SLOPE, feat, up) if ref is None else ref
    ins = [T(v, DEV).requires_grad_(True) for v in (feat, el.reshape(n_src, H, 1), er.reshape(n_dst, H, 1))]
    assert ops.gat_fused_supported(g, ins[0])
    out = ops.gat_fused(g, ins[0], ins[1], ins[2], SLOPE, 0.0, True)
    assert (g._index.csc().gat_tile_plan(F) is not None) == (tile == "1")
    got = N(out)
    assert np.isfinite(got).all(), ("gat_fused forward is not finite",) + what
    assert close_rows(got, ref["out"], ref["out_mag"]), ("gat_fused forward",) + what
    out.backward(T(up, DEV))
    d_feat, d_el, d_er = N(ins[0].grad), N(ins[1].grad).reshape(n_src, H), N(ins[2].grad).reshape(n_dst, H)
    assert np.isfinite(d_feat).all() and np.isfinite(d_el).all() and np.isfinite(d_er).all(), ("gat_fused backward is not finite",) + what
    assert close_rows(d_feat, ref["dfeat"], ref["dfeat_mag"]), ("gat_fused d feat",) + what
    assert close_rows(d_el, ref["del"], ref["del_mag"]), ("gat_fused d el",) + what
    assert close_rows(d_er, ref["der"], ref["der_mag"]), ("gat_fused d er",) + what
    if masked is not None:
        ms = np.zeros((n_src, H), bool)
        ms[src] = masked
        assert not d_el[ms].any() and not d_feat[ms].any(), ("gat_fused: gradients of a masked source must be exactly 0",) + what
    with torch.no_grad():
        a = ops.gat_attention(g, ins[1], ins[2], SLOPE)
        comp = N(ops.gspmm(g, "mul", "sum", ins[0], a.view(-1, H, 1)))
    assert close_rows(got, comp, 2 * ref["out_mag"]), ("gat_fused against gat_attention + gspmm",) + what
    return got, d_er


def fused_legs(H, F, monkeypatch):
    for mode, split, tile in LEGS:
        if tile == "1" and not (H == 1 and F % 4 == 0 and 4 <= F <= 16):
            continue
        set_leg(monkeypatch, mode, split, tile)
        g = graph_of(PRIVATE, torch.int32, DEV)
        plan = g._index.csc().plan()
        assert (plan is None) == (mode == "none") and (plan is None or plan.num_hubs >= 1)
        yield g, (mode, split, tile)


@pytest.mark.gpu
@pytest.mark.parametrize("H,F", [(1, 16), (4, 8), (1, 41)])
def test_fused_gat_layer_wide_range(H, F, monkeypatch):
    G = PRIVATE
    src, dst, n_src, n_dst = G
    feat, up = fused_operands(H, F, 70 + F)
    for g, leg in fused_legs(H, F, monkeypatch):
        for name in ve.PATTERNS:
            for rnd in rounds_for(name):
                z = ve.logit_pattern(name, dst, n_dst, H, 50 + H, rnd)
                el, er = split_er(z, dst, n_dst, 32)
                ref = memo(G, ("fused", name, rnd, H, F), lambda: ve.gat_reference(G, el, er, SLOPE, feat, up))
                run_fused(g, G, el, er, feat, up, (name, rnd, H, F) + leg, leg[2], ref=ref)


def masked_layer(H, F, rnd):
    """(el, er, feat, up, masked) of round `rnd`: logits AND features are dealt by rank among the unmasked edges of a row, so a row's
    exact result is the same for every placement of the masked edges; a masked source carries a finite feature (7.0)."""
    src, dst, n_src, n_dst = PRIVATE
    nnz = src.shape[0]
    deg = private_lens()
    z, masked = ve.masked_logits(dst, n_dst, H, 60, rnd)
    el, er = split_er(z, dst, n_dst, 32)
    pool, up = fused_operands(H, F, 80 + F)
    starts = (np.cumsum(deg) - deg)[dst]
    by_edge = np.empty((nnz, H, F), np.float32)
    for h in range(H):
        kept = ~masked[:, h]
        keep_rank = xl.rank_in_row(dst[kept], np.arange(int(kept.sum())))
        by_edge[kept, h] = pool[starts[kept] + keep_rank, h]
        by_edge[~kept, h] = 7.0
    feat = np.empty_like(by_edge)
    feat[src] = by_edge
    return el, er, feat, up, masked


@pytest.mark.gpu
@pytest.mark.parametrize("H,F", [(1, 16), (4, 8), (1, 41)])
def test_fused_gat_layer_masked_sources(H, F, monkeypatch):
    """el[u] = -inf masks a source.  Before the guard on the running maximum in gat_fused_kernel<FWD> and gat_tile.inc, a masked
    edge that OPENED a lane's stream (rank 0, a whole lane group's share, a whole first step or hub chunk) made
    __expf(-inf - -inf) = NaN and with it the whole output row; the same edge anywhere later gave the correct 0."""
    G = PRIVATE
    src, dst, n_src, n_dst = G
    deg = private_lens()
    seen = None
    for rnd in range(4):
        cov = masked_coverage(masked_layer(H, F, rnd)[4], dst, n_dst)
        seen = cov if seen is None else {k: seen[k] + cov[k] for k in cov}
    assert min(seen.values()) >= 1, seen
    for g, leg in fused_legs(H, F, monkeypatch):
        outs = []
        for rnd in range(4):
            el, er, feat, up, masked = masked_layer(H, F, rnd)
            ref = memo(G, ("fused masked", rnd, H, F), lambda: ve.gat_reference(G, el, er, SLOPE, feat, up))
            outs.append((run_fused(g, G, el, er, feat, up, ("masked", rnd, H, F) + leg, leg[2], masked=masked, ref=ref), ref))
        (out0, d_er0), ref0 = outs[0]
        for (out, d_er), ref in outs[1:]:                                   # every placement: the same rows within both bounds
            assert close_rows(out, out0, ref["out_mag"] + ref0["out_mag"]), ("the output depends on where the masked edges sit",) + leg
            assert close_rows(d_er, d_er0, ref["der_mag"] + ref0["der_mag"]), ("d er depends on where the masked edges sit",) + leg
        # fully masked rows (every second non-empty one): the other rows are unaffected
        el, er, feat, up, masked = masked_layer(H, F, 0)
        dead = (np.arange(n_dst) % 2 == 0) & (deg > 0)
        el = el.copy()
        el[src[dead[dst]]] = -np.inf
        with torch.no_grad():
            out = N(ops.gat_fused(g, T(feat, DEV), T(el.reshape(n_src, H, 1), DEV), T(er.reshape(n_dst, H, 1), DEV), SLOPE, 0.0, True))
        assert np.isfinite(out[~dead]).all() and close_rows(out[~dead], ref0["out"][~dead], ref0["out_mag"][~dead]), ("fully masked rows",) + leg


@pytest.mark.gpu
def test_fused_gat_nan_logit_in_a_hub_row_is_the_same_split_or_not(monkeypatch):
    """One NaN attention term el[u, 1] on an edge of the 1000-edge row.  The row kernel's rule (fmaxf: a NaN is never the maximum;
    1 / s = 0 unless s > 0) leaves (m finite, 1 / s = 0) in nstat for that row and head whether the row is walked whole or in hub
    chunks merged by hub_online_merge_kernel<false>, so the backward sees the same statistics in every leg: d feat is NaN at the
    NaN edge's source alone.  Merged under the dot-product family's rule (1 / s = NaN) the split legs would poison d feat of every
    source of the row.  The edge sits at storage rank 300: position 44 of its 64-edge step and of its chunk at both thresholds,
    never the first edge a lane group sees (a NaN that OPENS a stream meets m = -inf and counts for nothing, like a masked edge)."""
    src, dst, n_src, n_dst = PRIVATE
    H, F = 2, 8
    deg = private_lens()
    hub = int(np.argmax(deg))
    assert int(deg[hub]) == 1000
    u = int(src[np.nonzero(dst == hub)[0][300]])                            # edge-id order is storage order inside a row
    fed = ve.fed_rows(src, dst, n_dst, [u])
    assert np.array_equal(np.nonzero(fed)[0], [hub])
    rng = np.random.default_rng(77)
    feat, up = fused_operands(H, F, 78)
    el, er = rng.standard_normal((n_src, H)).astype(np.float32), rng.standard_normal((n_dst, H)).astype(np.float32)
    ref = ve.gat_reference(PRIVATE, el, er, SLOPE, feat, up)                # of the clean logits: the magnitudes of the bound
    el[u, 1] = np.nan
    want_nan = np.zeros((n_dst, H, F), bool)
    want_nan[fed, 1] = True
    legs = {}
    for mode, split in (("none", 256), ("natural", 64), ("natural", 256)):
        set_leg(monkeypatch, mode, split, "0")
        g = graph_of(PRIVATE, torch.int32, DEV)
        plan = g._index.csc().plan()
        assert (plan is None) == (mode == "none") and (plan is None or plan.num_hubs == int((deg > split).sum()) >= 1)
        assert g._index.csc().gat_tile_plan(F) is None
        ins = [T(v, DEV).requires_grad_(True) for v in (feat, el.reshape(n_src, H, 1), er.reshape(n_dst, H, 1))]
        out = ops.gat_fused(g, ins[0], ins[1], ins[2], SLOPE, 0.0, True)
        out.backward(T(up, DEV))
        got = dict(out=N(out), dfeat=N(ins[0].grad), **{"del": N(ins[1].grad).reshape(n_src, H), "der": N(ins[2].grad).reshape(n_dst, H)})
        assert np.array_equal(np.isnan(got["out"]), want_nan) and np.isfinite(got["out"][~want_nan]).all(), ("out", mode, split)
        legs[mode, split] = got
    first = legs["none", 256]
    for key, got in legs.items():
        for name in ("out", "dfeat", "del", "der"):
            nan = np.isnan(first[name])
            assert np.array_equal(np.isnan(got[name]), nan), ("the NaN mask of %s depends on the hub split" % name, key, int(np.isnan(got[name]).sum()), int(nan.sum()))
            assert np.isfinite(got[name][~nan]).all(), (name, key)
            assert close_rows(np.where(nan, 0, got[name]), np.where(nan, 0, first[name]), ref[name + "_mag"]), (name, key)
    assert int(np.isnan(first["dfeat"]).any(axis=(1, 2)).sum()) == 1 and np.isnan(first["dfeat"][u, 1]).all()


# ============================================================================= 4. a non-finite source stays where the graph sends it
_wired = {}


def wired_ladder():
    """The square ladder with two of its idle sources (the ladder's last 40 feed nobody) wired in: on the ladder itself every source
    that feeds anything feeds half of all rows (363 504 edges over 373 sources), so no source meets the 1 - 10 % condition.  Every
    12th row, the 21 000-edge hub row included, has one of its edges re-pointed to source n - 1 and every 12th row from row 5 on one
    to source n - 2: at the row's first, last or middle storage rank in turn.  Row lengths and edge order are the ladder's."""
    if "G" not in _wired:
        src, dst, n, _ = ladder(False)
        src = src.copy()
        rank = xl.rank_in_row(dst, np.arange(dst.shape[0]))
        lens = degrees((src, dst, n, n))
        for u, first in ((n - 1, 0), (n - 2, 5)):
            rows = np.arange(first, n, 12)
            rows = rows[lens[rows] > 0]
            spot = np.where(np.arange(rows.shape[0]) % 3 == 0, 0, np.where(np.arange(rows.shape[0]) % 3 == 1, lens[rows] - 1, lens[rows] // 2))
            at = np.full(n, -1)
            at[rows] = spot
            src[rank == at[dst]] = u
        _wired["G"] = (src, dst, n, n)
    return _wired["G"]


def isolation_case(G, D, bad, seed, check_share):
    """(X with source bad[0] = NaN and bad[1] = +inf, the int64 sums of the other rows, the mask of the rows those two feed)."""
    def make():
        src, dst, n_src, n_dst = G
        fed = ve.fed_rows(src, dst, n_dst, list(bad))
        if check_share:                                                     # from the COO list alone
            for u in bad:
                share = float(ve.fed_rows(src, dst, n_dst, [u]).mean())
                assert 0.01 <= share <= 0.10, (u, share)
        assert 0 < int(fed.sum()) < n_dst - 8
        X = ints(np.random.default_rng(seed + D), (n_src, D), 8)
        Xz = X.copy()
        Xz[list(bad)] = 0.0
        want = exact_pair(dst, n_dst, lambda c: Xz[:, c][src], D)
        X[bad[0]], X[bad[1]] = np.nan, np.inf
        return X, want, fed
    return memo(G, ("isolation", D, bad), make)


def assert_isolated(got, want, fed, deg, red, what):
    got = np.asarray(got).reshape(want.shape)
    wrong = ~np.isfinite(got) != fed[:, None]
    assert not wrong.any(), "%s: %d elements are non-finite where they must not be (or finite where a non-finite source is summed), first at %s" % (
        what, int(wrong.sum()), np.argwhere(wrong)[0].tolist())
    if red == "sum":
        xl.assert_exact(got[~fed], want[~fed], what)
    else:
        xl.assert_mean(got[~fed], want[~fed], deg[~fed], what)


ISOLATION_ROUNDS = (("wired", lambda n: (n - 1, n - 2), True), ("hub source", lambda n: (3, 0), False))


def isolation_graph(round_name):
    return wired_ladder() if round_name == "wired" else ladder(False)


def test_cpu_non_finite_sources_stay_in_their_rows(cpu_on):
    for round_name, pick, share in ISOLATION_ROUNDS:
        G = isolation_graph(round_name)
        deg = degrees(G)
        view = view_of(make_csr(G, torch.int32, "cpu"))
        for D in (1, 16, 100):
            X, want, fed = isolation_case(G, D, pick(G[2]), 90, share)
            for red in ("sum", "mean"):
                assert_isolated(N(sparse.gspmm_raw(view, "copy_lhs", red, T(X, "cpu"), None, dense_out=True)[0]), want, fed, deg, red,
                                "cpu copy_u %s D=%d %s" % (red, D, round_name))


@pytest.mark.gpu
@pytest.mark.parametrize("round_name,pick,share", ISOLATION_ROUNDS, ids=[r[0] for r in ISOLATION_ROUNDS])
def test_non_finite_sources_stay_in_their_rows_row_families(round_name, pick, share):
    """The wave-per-item kernels under every schedule (hub-split plans among them), the masked form, the lane-group kernel with and
    without a `rest` part, the edge-tail kernel and the multi-relation kernel."""
    G = isolation_graph(round_name)
    src, dst, n, _ = G
    deg = degrees(G)
    csr = make_csr(G, torch.int32, DEV)
    be = sparse.backend_for(csr.indptr)
    views = gpu_views(csr, splits=(64, 256))
    for D in (1, 16, 64, 100, 132):
        X, want, fed = isolation_case(G, D, pick(n), 90, share)
        x = T(X, DEV)
        for red in ("sum", "mean"):
            for name, v in views:
                what = "%s D=%d %s %s" % (red, D, name, round_name)
                assert_isolated(N(sparse.gspmm_raw(v, "copy_lhs", red, x, None, dense_out=True)[0]), want, fed, deg, red, "row " + what)
                assert last_kernel() == "rowwave32"
                if D % 4 == 0 and D <= 100:
                    bits_ = be.row_nonzero_bits(x)
                    assert_isolated(N(be.spmm_copy_u_masked(v, red, x, bits_)), want, fed, deg, red, "masked " + what)
                    assert last_kernel() == "rowwave32"
            if D in (16, 64, 100):
                for limit in (32, 5, None):                                 # two-part plans; None: every row by a lane group, no rest
                    v = view_of(csr, "natural", 256) if limit else view_of(csr)
                    if limit:
                        plan = schedule.split_short_items(v, v.plan(), any_share=True, limit=limit)[0]
                        assert plan.rest is not None
                    v._short = {nb: (plan if limit else True) for nb in GROUPS}
                    out = torch.full((n, D), 7.0, device=DEV)
                    be.spmm_copy_u_strided(v, red, x, out)
                    assert last_kernel() == "rowgroup32", (D, limit, last_kernel())
                    assert_isolated(N(out), want, fed, deg, red, "lane group limit=%s %s D=%d %s" % (limit, red, D, round_name))
        if D == 100:
            xw = torch.cat([x, torch.zeros_like(x)], 1)[:, :100]
            for name, v in views[:3]:
                a, tail = be.edge_tail_of(v, xw)
                for red in ("sum", "mean"):
                    out = torch.full((n, 100), 7.0, device=DEV)
                    be.spmm_copy_u_edge_tail(v, red, a, tail, out)
                    assert last_kernel() == "edge tail"
                    assert_isolated(N(out), want, fed, deg, red, "edge tail %s %s %s" % (red, name, round_name))
        if D in (1, 16, 64):                                                # rel: R = 3 relations of weight 1, 2 and -1: the same sums, scaled
            w = T(np.repeat(np.array([[1.0, 2.0, -1.0]], np.float32), src.shape[0], 0), DEV)
            for kind, split in (("none", 0), ("natural", 64)):
                v = view_of(csr, kind, split)
                for red in ("sum", "mean"):
                    out = N(be.spmm_rel(v, red, be.gather_rows(w, v.eids), x))
                    assert last_kernel() == "rel"
                    for r, f in enumerate((1, 2, -1)):
                        assert_isolated(out[:, r], f * want, fed, deg, red, "rel r=%d %s D=%d %s %s" % (r, red, D, kind, round_name))


@pytest.mark.gpu
@pytest.mark.parametrize("round_name,pick,share", ISOLATION_ROUNDS, ids=[r[0] for r in ISOLATION_ROUNDS])
def test_non_finite_sources_stay_in_their_rows_tile_and_slots(round_name, pick, share):
    G = isolation_graph(round_name)
    src, dst, n, _ = G
    deg = degrees(G)
    csr = make_csr(G, torch.int32, DEV)
    be = sparse.backend_for(csr.indptr)
    for lanes_log2, widths in ((4, (64, 100, 132)), (2, (16,))):            # tile and tile-narrow
        cfg = mgx_config.TILE_CONFIG[lanes_log2]
        plans = []
        for split, order in ((mgx_config.TILE_HUB_SPLIT, torch.randperm(n, generator=torch.Generator().manual_seed(5)).to(DEV)), (64, None)):
            base = schedule.build_plan(csr, order, split, "cluster")
            tp = tileplan.build_tile_plan(csr, base, *cfg, lanes_log2=lanes_log2)
            tileplan.validate(tp, csr)
            assert base.num_hubs >= 1 and tp.num_tiles >= 2
            plans.append((split, tp))
        for D in widths:
            if D % 4 or (lanes_log2 == 4 and D > 128):
                continue
            X, want, fed = isolation_case(G, D, pick(n), 90, share)
            for split, tp in plans:
                for red in ("sum", "mean"):
                    out = N(be.spmm_tile_copy_u(csr, tp, red, T(X, DEV)))
                    assert last_kernel() == "tile"
                    assert_isolated(out, want, fed, deg, red, "tile lg=%d split=%d %s D=%d %s" % (lanes_log2, split, red, D, round_name))
    # slots (D = 64): rows of at most 24 non-zeros travel as slots, the NaN row (64 NaNs) and the inf row as overflow rows
    bad = pick(n)
    X, _, fed = isolation_case(G, 64, bad, 90, share)
    X = np.where(np.random.default_rng(91).random(X.shape) < 0.3, X, np.float32(0.0))
    X[bad[0]], X[bad[1]] = np.nan, np.inf
    Xz = np.where(np.isfinite(X), X, 0).astype(np.float32)
    want = exact_pair(dst, n, lambda c: Xz[:, c][src], 64)
    x = T(X, DEV)
    assert be.rows_slots_supported(x, view_of(csr))
    slots, _ = be.rows_slots_pack(x)
    for name, v in gpu_views(csr, splits=(64, 256)):
        for red in ("sum", "mean"):
            out = torch.full((n, 64), 7.0, device=DEV)
            be.spmm_copy_u_strided(v, red, x, out, slots=slots)
            assert last_kernel() == "slots", name
            assert_isolated(N(out), want, fed, deg, red, "slots %s %s %s" % (red, name, round_name))


@pytest.mark.gpu
def test_non_finite_sources_u_mul_e_and_fused_gat(monkeypatch):
    """u_mul_e with per-head weights: a weight of exactly 0 on an edge from the inf source is 0 x inf = NaN in the reference too, so
    the reference (fp64 row sums with IEEE classes) decides which elements are non-finite.  gat_fused forward with one NaN feature
    row: NaN in the rows it feeds, every other row within the fused-layer bound."""
    G = wired_ladder()
    src, dst, n, _ = G
    bad = (n - 1, n - 2)
    fed = ve.fed_rows(src, dst, n, list(bad))
    csr = make_csr(G, torch.int32, DEV)
    rng = np.random.default_rng(95)
    for H, F in ((3, 4), (8, 8), (1, 64)):
        X, W = ints(rng, (n, H, F), 8), ints(rng, (src.shape[0], H, 1), 2)
        X[bad[0]], X[bad[1]] = np.nan, np.inf
        from_inf = src == bad[1]
        assert bool((W[from_inf] == 0).any()) and bool((W[from_inf] != 0).any())
        with np.errstate(invalid="ignore"):
            term = (X[src] * W).astype(np.float32).reshape(-1, H * F)
        want = ve.float_rows_sum(dst, n, term)
        assert np.array_equal(~np.isfinite(want).all(1), fed) and bool(np.isnan(want[fed]).any())
        for name, v in gpu_views(csr, splits=(64, 256)):
            got = N(sparse.gspmm_raw(v, "mul", "sum", T(X, DEV), T(W, DEV), dense_out=True)[0]).reshape(n, H * F)
            assert last_kernel() == "rowwave32"
            assert np.array_equal(np.isfinite(got), np.isfinite(want)), ("u_mul_e", H, F, name)
            assert np.array_equal(got[np.isfinite(want)], want[np.isfinite(want)].astype(np.float32)), ("u_mul_e", H, F, name)
    fused_nan_feature_cases(G, (bad[0], 0), 8, monkeypatch)
    # the private-source graph: every source is used once, so the tile walk takes all of them through its direct list, whose
    # padding entries name source 0 -- the one destination that source feeds is NaN, no other
    fused_nan_feature_cases(PRIVATE, (0, PRIVATE[0][-1]), 1, monkeypatch)


def fused_nan_feature_cases(G, nan_sources, least, monkeypatch):
    src, dst, n_src, n_dst = G
    rng = np.random.default_rng(96)
    for H, F in ((1, 16), (4, 8), (1, 41)):
        feat, up = rng.standard_normal((n_src, H, F)).astype(np.float32), rng.standard_normal((n_dst, H, F)).astype(np.float32)
        el, er = rng.standard_normal((n_src, H)).astype(np.float32), rng.standard_normal((n_dst, H)).astype(np.float32)
        ref = ve.gat_reference(G, el, er, SLOPE, feat, up)
        for nan_source in nan_sources:
            bad_feat = feat.copy()
            bad_feat[nan_source] = np.nan
            only = ve.fed_rows(src, dst, n_dst, [nan_source])
            assert least <= int(only.sum()) <= n_dst - 8
            for mode, split, tile in LEGS:
                if tile == "1" and not (H == 1 and F % 4 == 0 and 4 <= F <= 16):
                    continue
                set_leg(monkeypatch, mode, split, tile)
                g = graph_of(G, torch.int32, DEV)
                with torch.no_grad():
                    out = N(ops.gat_fused(g, T(bad_feat, DEV), T(el.reshape(n_src, H, 1), DEV), T(er.reshape(n_dst, H, 1), DEV), SLOPE, 0.0, True))
                what = (H, F, nan_source, mode, split, tile)
                assert (g._index.csc().gat_tile_plan(F) is not None) == (tile == "1")
                assert np.isnan(out[only]).all() and np.isfinite(out[~only]).all(), ("gat_fused NaN feature row",) + what
                assert close_rows(out[~only], ref["out"][~only], ref["out_mag"][~only]), ("gat_fused other rows",) + what
